// The guard every extern "C" entry point of capi.cpp runs under ("The C boundary").
// Host-only: no HIP header and nothing of the numeric layer, so a plain g++ test can include it.
#pragma once
#include <cstdint>
#include <cstring>
#include <memory>
#include <new>
#include <stdexcept>
#include <string>

#include "../../include/sparsecholesky.h"

namespace sc {

// what sc_last_error returns: the message of the last failing call on this thread
inline std::string& last_error() {
    static thread_local std::string s;
    return s;
}

inline const char* status_string(int64_t st) {
    if (st > 0) return "A is not positive definite.";  // chol.hpp:850
    switch (st) {
        case SC_OK: return "ok";
        case SC_ERR_ARG: return "invalid argument";
        case SC_ERR_NOMEM: return "host allocation failed";
        case SC_ERR_HIP: return "HIP runtime error";
        case SC_ERR_DEVMEM: return "device allocation failed";
        case SC_ERR_STATE: return "call out of order";
        case SC_ERR_COMM: return "communication error";
        case SC_ERR_NOTIMPL: return "not implemented";
        case SC_ERR_NOTSYM: return "matrix is not symmetric";
        case SC_ERR_IO: return "file could not be opened";
    }
    return "unknown status";
}

// a validator's failure: the reason without the entry point's name, which the guard adds
inline int64_t fail(const std::string& what, int64_t rc = SC_ERR_ARG) {
    last_error() = what;
    return rc;
}

// Runs f, which returns a status, and lets no exception out.  A status < 0 leaves
// "<who>: <reason>" in last_error(): the reason is what f left there (fail(), or a callee
// writing into last_error()), else sc_status_string's text; a reason that already begins with
// who is not prefixed again.  A status >= 0 leaves the stored message as it was.
template <class F>
int64_t guarded(const char* who, F&& f) noexcept {
    std::string& e = last_error();
    std::string kept;
    kept.swap(e);  // e is empty now: whatever it holds after f() is f's own
    int64_t rc = SC_ERR_STATE;
    try {
        try {
            rc = f();
        } catch (const std::exception& x) {
            const bool nomem = dynamic_cast<const std::bad_alloc*>(&x) || dynamic_cast<const std::length_error*>(&x);
            rc = nomem ? SC_ERR_NOMEM : SC_ERR_STATE;
            e = nomem ? std::string() : std::string("unexpected exception: ") + x.what();
        } catch (...) {
            rc = SC_ERR_STATE;
            e = "unexpected exception: unknown";
        }
        if (rc >= 0) {
            e.swap(kept);
        } else {
            if (e.empty()) e = status_string(rc);
            if (e.compare(0, std::strlen(who), who) != 0) e.insert(0, std::string(who) + ": ");
        }
    } catch (...) {
        e.clear();  // no memory even for the message: the status stands alone
    }
    return rc;
}

// The handle form, for a handle with a std::string err (sc::Numeric, sc::Normal): err is cleared
// before f, so that a failure without a message of its own does not show an earlier one, and is
// the reason afterwards unless f left one in last_error().
template <class H, class F>
int64_t guarded(const char* who, H& h, F&& f) noexcept {
    return guarded(who, [&]() -> int64_t {
        h.err.clear();
        const int64_t rc = f();
        if (rc < 0 && last_error().empty()) last_error() = h.err;
        return rc;
    });
}

// Creates a handle: allocates the wrapper W, runs create(W&) under the guard, frees the wrapper
// on any failure and stores *out only on success (*out is null otherwise).
template <class W, class F>
int64_t guarded_create(const char* who, W** out, F&& create) noexcept {
    return guarded(who, [&]() -> int64_t {
        if (!out) return fail("null out");
        *out = nullptr;
        std::unique_ptr<W> w(new W());
        const int64_t rc = create(*w);
        if (rc == SC_OK) *out = w.release();
        return rc;
    });
}

// for the entry points that return no status: f's value, or `otherwise` when f throws
template <class T, class F>
T guarded_or(T otherwise, F&& f) noexcept {
    try {
        return f();
    } catch (...) {
        return otherwise;
    }
}

}  // namespace sc
