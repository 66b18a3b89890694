// command_stream.h — the checked command stream of the diagnostics (bgs_diag.hip): a hook's memsets, copies, launch
// checks and its final wait on one HIP stream. The first command that fails is remembered, HIP's sticky error is cleared
// there, and nothing is issued behind it: every method is a no-op that returns false once `ok` is false. A launch, or any
// other HIP call the stream has no method for, goes under `if (cs.ok)` and hands its result to check() / launched().
#pragma once
#include <hip/hip_runtime.h>

namespace bgs_host {

struct CommandStream {
    hipStream_t st;
    bool ok = true;
    explicit CommandStream(hipStream_t stream) : st(stream) {}

    bool check(hipError_t e) {   // the result of a call made under `if (cs.ok)`
        if (e != hipSuccess && ok) { ok = false; (void)hipGetLastError(); }
        return ok;
    }
    bool fill(void* dev, int byte, size_t bytes) { return ok && check(hipMemsetAsync(dev, byte, bytes, st)); }
    bool zero(void* dev, size_t bytes) { return fill(dev, 0, bytes); }
    bool word(uint32_t* dev, uint32_t value) { return ok && check(hipMemsetD32Async((hipDeviceptr_t)dev, (int)value, 1, st)); }
    bool up(void* dev, const void* host, size_t bytes) { return ok && check(hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, st)); }
    bool down(void* host, const void* dev, size_t bytes) { return ok && check(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, st)); }
    // behind the launches made under `if (cs.ok)`; `launch`: what a launcher that reports an error of its own returned
    bool launched(hipError_t launch = hipSuccess) { return ok && check(launch) && check(hipGetLastError()); }
    bool sync() { return ok && check(hipStreamSynchronize(st)); }
};

}  // namespace bgs_host
