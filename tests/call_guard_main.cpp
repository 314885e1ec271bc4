// The call guard of the resident-index entry points (lm::guarded, lexicmap_amd/csrc/lm_internal.h) as a stand-alone program
// over a FAKE device, meant to be built with -fsanitize=address,undefined (tests/test_call_guard_cpu.py): a host-built
// lm_index, bodies that return or throw each kind of exception the guard maps, and after every call the status, the exact
// text on the handle and a free mutex.  The LM_ERR_NOMEM answers are checked here only: no GPU test exhausts a device.
// Test infrastructure only.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <new>
#include <thread>

namespace fake {
static int set_device_calls = 0, last_device = -1, last_error_calls = 0;
static bool set_device_fails = false;
static hipError_t SetDevice(int d) {
    set_device_calls++;
    last_device = d;
    return set_device_fails ? hipErrorInvalidDevice : hipSuccess;
}
static hipError_t GetLastError() {
    last_error_calls++;
    return hipSuccess;
}
static hipError_t Refuse(void **p) {
    *p = nullptr;
    return hipErrorOutOfMemory;
}
static hipError_t Ok() { return hipSuccess; }
static const char *ErrStr(hipError_t e) { return e == hipSuccess ? "ok" : e == hipErrorOutOfMemory ? "fake out of memory" : "fake invalid device"; }
} // namespace fake

#define hipSetDevice(d) fake::SetDevice(d)
#define hipMalloc(p, n) fake::Refuse((void **)(p))
#define hipFree(p) fake::Ok()
#define hipMemGetInfo(a, b) fake::Ok()
#define hipGetLastError() fake::GetLastError()
#define hipDeviceSynchronize() fake::Ok()
#define hipStreamSynchronize(s) fake::Ok()
#define hipStreamDestroy(s) fake::Ok()
#define hipMemsetAsync(p, v, n, s) fake::Ok()
#define hipGetErrorString(e) fake::ErrStr(e)
#define hipHostMalloc(p, n, f) fake::Refuse((void **)(p))
#define hipHostFree(p) fake::Ok()

#include "../lexicmap_amd/csrc/lm_internal.h"

static int checks = 0, failures = 0;
#define CHECK(cond)                                                              \
    do {                                                                         \
        checks++;                                                                \
        if (!(cond)) {                                                           \
            failures++;                                                          \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);             \
        }                                                                        \
    } while (0)

static const char *NOMEM = "the_call: the host could not hold it";

// the mutex is free: a lock attempt of this thread succeeds (and is given back)
static bool mutex_free(lm_index *ix) {
    if (!ix->mu.try_lock()) return false;
    ix->mu.unlock();
    return true;
}
// one guarded call whose body throws `ex`: the status, the exact text, a free mutex afterwards
template <class Ex> static void expect(lm_index *ix, const Ex &ex, lm_status want, const char *text) {
    const int sd = fake::set_device_calls;
    const lm_status got = lm::guarded(ix, NOMEM, [&]() { throw ex; });
    CHECK(got == want);
    CHECK(ix->err == text);
    CHECK(fake::set_device_calls == sd + 1 && fake::last_device == ix->device);
    CHECK(mutex_free(ix));
}

int main() {
    lm_index *ix = new lm_index();
    ix->device = 3;

    // ---- a body that returns: LM_OK, run once, under the mutex, on the handle's device; the text is left alone
    ix->err = "text of an earlier call";
    int ran = 0;
    bool held = false;
    lm_status st = lm::guarded(ix, NOMEM, [&]() {
        ran++;
        std::thread t([&] { // (another thread: this one owns the mutex)
            held = !ix->mu.try_lock();
            if (!held) ix->mu.unlock();
        });
        t.join();
    });
    CHECK(st == LM_OK && ran == 1 && held);
    CHECK(fake::set_device_calls == 1 && fake::last_device == 3);
    CHECK(ix->err == "text of an earlier call");
    CHECK(mutex_free(ix));

    // ---- every arm, twice over in two orders: a later failure shows its own text whole, nothing of the one before
    for (int round = 0; round < 2; round++) {
        expect(ix, lm::ArgError("the_call: keys is NULL but nkeys is not 0"), LM_ERR_ARG, "the_call: keys is NULL but nkeys is not 0");
        expect(ix, lm::OptionError("the_call: min_prefix (99) should be in the range of [12, 31]"), LM_ERR_OPTION,
               "the_call: min_prefix (99) should be in the range of [12, 31]");
        const int le = fake::last_error_calls;
        expect(ix, lm::DeviceOOM("the_call: 7 tuples need 34 B each: device scratch allocation failed"), LM_ERR_NOMEM,
               "the_call: 7 tuples need 34 B each: device scratch allocation failed"); // not LM_ERR_HIP: a DeviceOOM is a HipError
        CHECK(fake::last_error_calls == le + 1);                                       // the sticky device error is cleared
        expect(ix, std::bad_alloc(), LM_ERR_NOMEM, NOMEM);
        CHECK(fake::last_error_calls == le + 1);
        expect(ix, lm::HipError("hipMemcpyAsync(..): fake failure at file:1"), LM_ERR_HIP, "hipMemcpyAsync(..): fake failure at file:1");
        expect(ix, std::runtime_error("the_call: a piece does not fit its plan"), LM_ERR_HIP, "the_call: a piece does not fit its plan");
        expect(ix, std::bad_alloc(), LM_ERR_NOMEM, NOMEM);        // a short text after a longer one
        expect(ix, lm::ArgError(""), LM_ERR_ARG, "");             // and an empty one
        expect(ix, std::length_error("vector::reserve"), LM_ERR_HIP, "vector::reserve"); // any other std::exception
    }

    // ---- a DeviceOOM a real allocation throws (DBuf over the refusing fake device) and one wrapped with sizes, as the calls do
    st = lm::guarded(ix, NOMEM, [&]() {
        lm::DBuf<uint64_t> d;
        try {
            d.alloc_exact(1000);
        } catch (const lm::DeviceOOM &e) {
            throw lm::DeviceOOM(std::string("the_call: 1000 keys need 8 B each: ") + e.what());
        }
    });
    CHECK(st == LM_ERR_NOMEM);
    CHECK(ix->err == "the_call: 1000 keys need 8 B each: device allocation of 0 MB failed: out of memory");
    CHECK(mutex_free(ix));

    // ---- the host's text given as the call's name and the rest (put together in the arm only)
    st = lm::guarded(ix, "lm_index_the_call", ": the host could not hold the plan", [&]() { throw std::bad_alloc(); });
    CHECK(st == LM_ERR_NOMEM);
    CHECK(ix->err == "lm_index_the_call: the host could not hold the plan");
    st = lm::guarded(ix, "lm_index_the_call", ": the host could not hold the plan", [&]() { throw lm::ArgError("lm_index_the_call: n is 0"); });
    CHECK(st == LM_ERR_ARG && ix->err == "lm_index_the_call: n is 0");
    CHECK(mutex_free(ix));

    // ---- hipSetDevice refused: the body does not run, LM_ERR_HIP with HIPCHK's text, the mutex free
    fake::set_device_fails = true;
    ran = 0;
    st = lm::guarded(ix, NOMEM, [&]() { ran++; });
    fake::set_device_fails = false;
    CHECK(st == LM_ERR_HIP && ran == 0);
    CHECK(ix->err.find("hipSetDevice(ix->device): fake invalid device at ") == 0);
    CHECK(mutex_free(ix));

    // ---- and the handle still answers
    ran = 0;
    st = lm::guarded(ix, NOMEM, [&]() { ran++; });
    CHECK(st == LM_OK && ran == 1);
    CHECK(mutex_free(ix));

    // ---- the helpers that moved beside the guard
    CHECK(lm::grid_for(0) == 1 && lm::grid_for(1) == 1 && lm::grid_for(256) == 1 && lm::grid_for(257) == 2 && lm::grid_for(100, 64) == 2);
    CHECK(lm::grid_for((int64_t)1 << 40) == 1 << 30);
    CHECK(lm::bits_for(0) == 1 && lm::bits_for(2) == 1 && lm::bits_for(3) == 2 && lm::bits_for(4) == 2 && lm::bits_for(5) == 3);
    CHECK(lm::bits_for((int64_t)1 << 31) == 31 && lm::bits_for(((int64_t)1 << 31) + 1) == 32);

    delete ix;
    printf("%s: %d checks, %d failed\n", failures ? "FAILED" : "ok", checks, failures);
    return failures ? 1 : 0;
}
