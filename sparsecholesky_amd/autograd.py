"""Differentiable log det A and inv(A) B over the GPU factorization (torch.autograd).

    chol = SparseCholesky(symb)          # owns one Numeric
    F = chol(values)                     # factors; a view bound to this factorization
    loss = F.logdet() + (F.solve(B) * M).sum()
    loss.backward()                      # values.grad, B.grad

``values`` is a float64 CUDA vector in the order :meth:`Numeric.factor` takes; its gradient has
the same length and order, zero on the slots the analysis ignores
(:meth:`Symbolic.value_entries`).  A stored entry stands for both mirrored positions of the
symmetric matrix, so the gradient of an off-diagonal slot is the sum over both.

Both functions of a view share its one factorization.  The handle holds one factor at a time:
factoring other values (calling the object again) or updating the factor retires every earlier
view, and a forward or backward pass through a retired view raises ``RuntimeError`` instead of
using the wrong factor.  Double backward is not supported.

This module imports torch; the package itself does not.
"""
import torch
from torch.autograd.function import once_differentiable

from . import LibraryError, Numeric, Symbolic

__all__ = ["SparseCholesky", "Factorization"]


def _check_tensor(t, what: str, shape=None):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float64):
        raise ValueError(f"{what} must be a float64 tensor on the GPU")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{what} is {tuple(t.shape)}, expected {tuple(shape)}")


def _sync(t: torch.Tensor):
    # the library works on its own stream and its calls are synchronous: what torch has
    # queued for the arrays must be done before the pointers are handed over
    torch.cuda.current_stream(t.device).synchronize()


class SparseCholesky:
    """Owns one :class:`Numeric` of ``symb``; calling it with a value tensor factors and
    returns the :class:`Factorization` view of that generation."""

    def __init__(self, symb: Symbolic, device: int = -1):
        self.symb = symb
        self.numeric = Numeric(symb, device=device)
        self.generation = 0
        self.nvalues = int(symb.A.p[symb.n]) if symb.n > 0 else 0

    def __call__(self, values: torch.Tensor) -> "Factorization":
        _check_tensor(values, "values", (self.nvalues,))
        v = values.contiguous()
        _sync(v)
        self.generation += 1  # whatever happens next, the earlier factor is gone
        st = self.numeric.factor_device(v.data_ptr())
        if st > 0:
            raise LibraryError(f"factor: A is not positive definite (column {st})")
        return Factorization(self, values)

    def _updown(self, W, sign: int) -> int:
        self.generation += 1
        return self.numeric.updown(W, sign)

    def update(self, W) -> int:
        """:meth:`Numeric.update`; the factor then belongs to another matrix than any view's
        values, so every view is retired."""
        return self._updown(W, +1)

    def downdate(self, W) -> int:
        return self._updown(W, -1)


class Factorization:
    """One factorization of a :class:`SparseCholesky`: ``logdet()`` and ``solve(B)``,
    differentiable with respect to the values (and B)."""

    def __init__(self, owner: SparseCholesky, values: torch.Tensor):
        self.owner = owner
        self.values = values
        self.generation = owner.generation

    def _live(self, what: str) -> Numeric:
        if self.generation != self.owner.generation:
            raise RuntimeError(
                f"{what}: this view belongs to factorization {self.generation} of its handle, which now holds "
                f"factorization {self.owner.generation} (the values were refactored or the factor was updated)")
        return self.owner.numeric

    def logdet(self) -> torch.Tensor:
        return _LogDet.apply(self.values, self)

    def solve(self, B: torch.Tensor) -> torch.Tensor:
        """X = inv(A) B for B (n,) or (n, k)."""
        n = self.owner.symb.n
        _check_tensor(B, "B")
        if B.ndim not in (1, 2) or B.shape[0] != n:
            raise ValueError(f"solve: B is {tuple(B.shape)}, the matrix has {n} rows")
        return _Solve.apply(self.values, B, self)


def _rows(T: torch.Tensor) -> torch.Tensor:
    """(n,) or (n, k) as a contiguous (k, n) tensor: the column-major panel the library takes."""
    return (T.reshape(-1, 1) if T.ndim == 1 else T).t().contiguous()


class _LogDet(torch.autograd.Function):
    @staticmethod
    def forward(ctx, values, view):
        num = view._live("logdet")
        ctx.view = view
        return values.new_tensor(num.logdet())

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        view = ctx.view
        num = view._live("backward of logdet")
        G = torch.empty(max(view.owner.nvalues, 1), dtype=torch.float64, device=g.device)
        _sync(G)
        num.logdet_grad_device(G.data_ptr())
        return g * G[:view.owner.nvalues], None


class _Solve(torch.autograd.Function):
    @staticmethod
    def forward(ctx, values, B, view):
        num = view._live("solve")
        n = view.owner.symb.n
        Bt = _rows(B)
        k = Bt.shape[0]
        Xt = torch.empty_like(Bt)
        _sync(Bt)
        if n > 0 and k > 0:
            st = num.solve_device_multi(Bt.data_ptr(), k, n, Xt.data_ptr(), n)
            if st > 0:
                raise LibraryError(f"solve: A is not positive definite (column {st})")
        ctx.view = view
        ctx.one = B.ndim == 1
        ctx.save_for_backward(Xt)
        return Xt[0].clone() if ctx.one else Xt.t()

    @staticmethod
    @once_differentiable
    def backward(ctx, gX):
        view = ctx.view
        num = view._live("backward of solve")
        (Xt,) = ctx.saved_tensors
        n, nv = view.owner.symb.n, view.owner.nvalues
        Gt = _rows(gX)
        k = Gt.shape[0]
        Bbar = torch.empty_like(Gt)
        G = torch.empty(max(nv, 1), dtype=torch.float64, device=gX.device)
        _sync(G)
        num.solve_grad_device(Gt.data_ptr(), Xt.data_ptr(), k, n, n, Bbar.data_ptr(), n, G.data_ptr())
        gB = Bbar[0].clone() if ctx.one else Bbar.t()
        return (G[:nv] if ctx.needs_input_grad[0] else None), (gB if ctx.needs_input_grad[1] else None), None
