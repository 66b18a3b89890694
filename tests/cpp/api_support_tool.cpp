// api_support_tool.cpp — TEST-ONLY stand-alone program over the host code the small libraries' C ABI files share
// (bevy_gaussian_splatting_amd/small_lib/api_support.h, the part without HIP), built by tests/test_native_binding.py with
// the address and undefined-behaviour sanitizers and run as a process of its own.
//
// It checks the error buffer (a message longer than it is cut at 511 characters and terminated; a second failure replaces
// the first) and the validation of a list of planes (NULL, misaligned, an output that is another plane as well; two equal
// inputs are fine), prints one line per case as `status message`, and returns 1 at the first answer that is not the
// expected one.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>

#include "../../bevy_gaussian_splatting_amd/small_lib/api_support.h"

static void expect(const char* what, int status, int want_status, const std::string& want_message) {
    printf("%d %s\n", status, g_error);
    if (status != want_status || want_message != g_error) {
        fprintf(stderr, "api_support_tool: %s: got %d \"%s\", expected %d \"%s\"\n", what, status, g_error, want_status, want_message.c_str());
        exit(1);
    }
}

int main() {
    static_assert(sizeof g_error == 512 && API_EINVAL == -1 && API_ENOMEM == -2 && API_EHIP == -3, "the buffer and the status codes");

    // ---- the error buffer ----
    const std::string longer(600, 'x');
    memset(g_error, '#', sizeof g_error);
    expect("a message longer than the buffer", fail(API_EHIP, "fn: %s", longer.c_str()), API_EHIP, "fn: " + std::string(507, 'x'));
    if (strlen(g_error) != 511 || g_error[511] != 0) {
        fprintf(stderr, "api_support_tool: the cut message is %zu characters\n", strlen(g_error));
        return 1;
    }
    expect("a second failure replaces the first", fail(API_ENOMEM, "second %d", 2), API_ENOMEM, "second 2");

    // ---- the planes: three inputs, then two outputs ----
    alignas(16) static char memory[5 * 16];
    const char* const names[5] = {"in_a", "in_b", "in_c", "out_a", "out_b"};
    Named good[5];
    for (int k = 0; k < 5; ++k) good[k] = {names[k], memory + 16 * k};
    g_error[0] = 0;
    expect("five distinct aligned planes", check_planes("fn", good, 3, 5), 0, "");

    for (int k : {0, 2, 4}) {   // the first, a middle and the last plane
        Named planes[5];
        memcpy(planes, good, sizeof good);
        planes[k].ptr = nullptr;
        expect("a NULL plane", check_planes("fn", planes, 3, 5), API_EINVAL, std::string("fn: ") + names[k] + " is NULL");
    }
    for (int k : {1, 3}) {
        Named planes[5];
        memcpy(planes, good, sizeof good);
        planes[k].ptr = memory + 16 * k + 8;
        expect("an address off by 8", check_planes("fn", planes, 3, 5), API_EINVAL,
               std::string("fn: ") + names[k] + " must be a 16-byte aligned device address");
    }
    {
        // plane by plane, both checks: a misaligned plane is named before a NULL one that stands later in the list
        Named planes[5];
        memcpy(planes, good, sizeof good);
        planes[1].ptr = memory + 16 + 8;
        planes[3].ptr = nullptr;
        expect("the first offender", check_planes("fn", planes, 3, 5), API_EINVAL, "fn: in_b must be a 16-byte aligned device address");
    }
    {
        Named planes[5];
        memcpy(planes, good, sizeof good);
        planes[3].ptr = good[1].ptr;
        expect("an output that is an input", check_planes("fn", planes, 3, 5), API_EINVAL, "fn: out_a is in_b as well");
        planes[3].ptr = good[3].ptr;
        planes[4].ptr = good[3].ptr;
        expect("an output that is an earlier output", check_planes("fn", planes, 3, 5), API_EINVAL, "fn: out_b is out_a as well");
    }
    {
        Named planes[5];
        memcpy(planes, good, sizeof good);
        planes[2].ptr = good[0].ptr;
        g_error[0] = 0;
        expect("two inputs that are the same plane", check_planes("fn", planes, 3, 5), 0, "");
    }
    expect("no plane at all", check_planes("fn", good, 0, 0), 0, "");
    return 0;
}
