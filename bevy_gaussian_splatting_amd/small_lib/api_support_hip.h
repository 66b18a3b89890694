// api_support_hip.h — the HIP side of what the C ABI files of the small device libraries share, over api_support.h: a
// failed HIP call as the last error, the device scope of a call, and the check of a device's number. Host code only,
// included by a library's *_api.hip and by nothing else.
#pragma once
#include <hip/hip_runtime.h>

#include "api_support.h"

namespace {

int fail_hip(const char* what, hipError_t e) { return fail(API_EHIP, "%s: %s", what, hipGetErrorString(e)); }

// Makes `device` current for the calling thread and puts the previous one back: the host's own choice is not disturbed.
class DeviceScope {
  public:
    explicit DeviceScope(int device) {
        if (hipGetDevice(&previous_) != hipSuccess) previous_ = -1;
        status_ = hipSetDevice(device);
    }
    ~DeviceScope() {
        if (status_ == hipSuccess && previous_ >= 0) (void)hipSetDevice(previous_);
    }
    hipError_t status() const { return status_; }

  private:
    int previous_ = -1;
    hipError_t status_ = hipSuccess;
};

// 0 if `hip_device` names a device this process can see; a negative number is API_EINVAL, any other API_EHIP.
int check_device(const char* fn, int hip_device) {
    if (hip_device < 0) return fail(API_EINVAL, "%s: hip_device %d", fn, hip_device);
    int devices = 0;
    if (hipGetDeviceCount(&devices) != hipSuccess || hip_device >= devices)
        return fail(API_EHIP, "%s: no usable HIP device %d (%d visible)", fn, hip_device, devices);
    return 0;
}

}  // namespace
