// api_support.h — what the C ABI files of the small device libraries share and that needs no HIP: the calling thread's
// last error, and the validation of a list of device planes. Host code only, included by a library's *_api.hip and by
// nothing else (never by a kernels file). Everything is in the anonymous namespace: each library has its own copy of
// the error buffer. tests/cpp/api_support_tool.cpp runs this header under the sanitizers.
#pragma once
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

namespace {

// The status codes every small library's header gives these names; its *_api.hip static_asserts that they are its own.
constexpr int API_EINVAL = -1, API_ENOMEM = -2, API_EHIP = -3;

thread_local char g_error[512] = "";

// Writes the message (cut to the buffer) over the previous one and returns `status`, so that a refusal is one line.
int fail(int status, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof g_error, fmt, ap);
    va_end(ap);
    return status;
}

struct Named {
    const char* name;
    const void* ptr;
};

// `planes` holds `count` device planes, the first `inputs` of them read and the rest written. 0, or API_EINVAL with
// the first offender named: a plane that is NULL or not 16-byte aligned, then an output that is an earlier plane as
// well. Two inputs may be the same plane.
int check_planes(const char* fn, const Named* planes, int inputs, int count) {
    for (int k = 0; k < count; ++k) {
        if (!planes[k].ptr) return fail(API_EINVAL, "%s: %s is NULL", fn, planes[k].name);
        if ((uintptr_t)planes[k].ptr & 15u) return fail(API_EINVAL, "%s: %s must be a 16-byte aligned device address", fn, planes[k].name);
    }
    for (int o = inputs; o < count; ++o)
        for (int k = 0; k < o; ++k)
            if (planes[o].ptr == planes[k].ptr) return fail(API_EINVAL, "%s: %s is %s as well", fn, planes[o].name, planes[k].name);
    return 0;
}

}  // namespace
