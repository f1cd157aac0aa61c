// The guard of the C boundary (sparsecholesky_amd/csrc/capi_guard.hpp) alone, host-only: built with
// -fsanitize=address,undefined and run as a program of its own by tests/test_capi_boundary.py.
#include <new>
#include <stdexcept>
#include <string>

#include "../../sparsecholesky_amd/csrc/capi_guard.hpp"
#include "mini_test.hpp"

using sc::guarded;
using sc::last_error;

static int64_t run(const char* who, int64_t rc, const char* msg = nullptr) {
    return guarded(who, [&]() -> int64_t {
        if (msg) last_error() = msg;
        return rc;
    });
}

TEST(Guard, SuccessKeepsTheStoredMessage) {
    last_error() = "sc_before: earlier";
    EXPECT_EQ(run("sc_ok", 0), 0);
    EXPECT_EQ(last_error(), "sc_before: earlier");
    EXPECT_EQ(run("sc_npd", 7), 7);  // not positive definite, a count: not a failure
    EXPECT_EQ(last_error(), "sc_before: earlier");
    EXPECT_EQ(run("sc_ok", 0, "a message that a succeeding call leaves is dropped"), 0);
    EXPECT_EQ(last_error(), "sc_before: earlier");
}

TEST(Guard, FailureNamesTheEntryPoint) {
    last_error() = "sc_before: earlier";
    EXPECT_EQ(run("sc_f", SC_ERR_ARG, "null X"), SC_ERR_ARG);
    EXPECT_EQ(last_error(), "sc_f: null X");
    EXPECT_EQ(run("sc_f", SC_ERR_STATE, "sc_f: no factorization yet"), SC_ERR_STATE);  // named already
    EXPECT_EQ(last_error(), "sc_f: no factorization yet");
    EXPECT_EQ(run("sc_g", SC_ERR_ARG), SC_ERR_ARG);  // no message of its own: never the earlier one
    EXPECT_EQ(last_error(), "sc_g: invalid argument");
    EXPECT_EQ(run("sc_g", SC_ERR_DEVMEM), SC_ERR_DEVMEM);
    EXPECT_EQ(last_error(), "sc_g: device allocation failed");
    EXPECT_EQ(sc::fail("why"), SC_ERR_ARG);
    EXPECT_EQ(guarded("sc_h", [] { return sc::fail("k < 0"); }), SC_ERR_ARG);
    EXPECT_EQ(last_error(), "sc_h: k < 0");
}

TEST(Guard, ExceptionsBecomeStatuses) {
    EXPECT_EQ(guarded("sc_a", []() -> int64_t { throw std::bad_alloc(); }), SC_ERR_NOMEM);
    EXPECT_EQ(last_error(), "sc_a: host allocation failed");
    EXPECT_EQ(guarded("sc_b", []() -> int64_t { throw std::length_error("vector"); }), SC_ERR_NOMEM);
    EXPECT_EQ(last_error(), "sc_b: host allocation failed");
    EXPECT_EQ(guarded("sc_c", []() -> int64_t { throw std::runtime_error("boom"); }), SC_ERR_STATE);
    EXPECT_EQ(last_error(), "sc_c: unexpected exception: boom");
    EXPECT_EQ(guarded("sc_d", []() -> int64_t { throw 42; }), SC_ERR_STATE);
    EXPECT_EQ(last_error(), "sc_d: unexpected exception: unknown");
    // a half-written message does not survive the exception
    EXPECT_EQ(guarded("sc_e", []() -> int64_t { last_error() = "half"; throw std::bad_alloc(); }), SC_ERR_NOMEM);
    EXPECT_EQ(last_error(), "sc_e: host allocation failed");
    EXPECT_EQ(sc::guarded_or(-1.0, []() -> double { throw std::runtime_error("boom"); }), -1.0);
    EXPECT_EQ(sc::guarded_or(-1.0, [] { return 2.5; }), 2.5);
}

struct Handle {
    std::string err;
};

TEST(Guard, HandleFormCarriesTheHandlesMessage) {
    Handle h;
    h.err = "stale: from an earlier call";
    EXPECT_EQ(guarded("sc_f", h, [&]() -> int64_t { return SC_ERR_STATE; }), SC_ERR_STATE);
    EXPECT_EQ(last_error(), "sc_f: call out of order");  // err was cleared before the call
    EXPECT_EQ(guarded("sc_f", h, [&]() -> int64_t { return h.err = "hipMalloc failed", SC_ERR_DEVMEM; }), SC_ERR_DEVMEM);
    EXPECT_EQ(last_error(), "sc_f: hipMalloc failed");
    EXPECT_EQ(guarded("sc_f", h, [&]() -> int64_t { return h.err = "sc_f: named below", SC_ERR_ARG; }), SC_ERR_ARG);
    EXPECT_EQ(last_error(), "sc_f: named below");
    EXPECT_EQ(guarded("sc_f", h, [&]() -> int64_t { return h.err = "not a failure", 3; }), 3);
    EXPECT_EQ(last_error(), "sc_f: named below");
    EXPECT_EQ(guarded("sc_f", h, [&]() -> int64_t { return sc::fail("the validator's reason wins"); }), SC_ERR_ARG);
    EXPECT_EQ(last_error(), "sc_f: the validator's reason wins");
    EXPECT_EQ(guarded("sc_f", h, [&]() -> int64_t { throw std::bad_alloc(); }), SC_ERR_NOMEM);
}

struct Wrapper {
    int* payload = nullptr;
    ~Wrapper() { delete payload; }
};

TEST(Guard, CreateFreesTheWrapperOnFailure) {
    Wrapper* out = reinterpret_cast<Wrapper*>(0x10);
    // the creator fails after allocating: the leak check of the sanitizer sees a wrapper kept
    EXPECT_EQ(sc::guarded_create("sc_new", &out, [](Wrapper& w) { return w.payload = new int(1), sc::fail("bad m"); }),
              SC_ERR_ARG);
    EXPECT_TRUE(out == nullptr);
    EXPECT_EQ(last_error(), "sc_new: bad m");
    out = reinterpret_cast<Wrapper*>(0x10);
    EXPECT_EQ(sc::guarded_create("sc_new", &out,
                                 [](Wrapper& w) -> int64_t { w.payload = new int(2); throw std::length_error("big"); }),
              SC_ERR_NOMEM);
    EXPECT_TRUE(out == nullptr);
    EXPECT_EQ(sc::guarded_create("sc_new", &out, [](Wrapper& w) { return w.payload = new int(3), (int64_t)SC_OK; }), SC_OK);
    ASSERT_TRUE(out != nullptr && out->payload && *out->payload == 3);
    delete out;
    EXPECT_EQ(sc::guarded_create("sc_new", static_cast<Wrapper**>(nullptr), [](Wrapper&) { return (int64_t)SC_OK; }),
              SC_ERR_ARG);
    EXPECT_EQ(last_error(), "sc_new: null out");
}

int main(int argc, char** argv) { return mini::run_all(argc, argv); }
