// sb_error.h -- the one error idiom of the library: fail with a message, HIP call or fail, propagate a status.  The message goes to
// the object the call was made on (sb_last_error / sb_batch_last_error); sb_set_error is overloaded per object type (sb_engine.h,
// sb_batch.h) and falls back to the thread's create-error where the object is null.  HIP-free unless SB_HIP is used.
#pragma once
#include <cstddef>
#include <cstdio>

#include "../../include/softbody.h"

void sb_set_create_error(const char *msg); // sb_api.hip: what sb_last_error(NULL) returns
inline void sb_set_error(std::nullptr_t, const char *text) { sb_set_create_error(text); } // (calls without an object: the partitioner)

#define SB_FAIL(obj, code, ...)                       \
    do {                                              \
        char _buf[512];                               \
        snprintf(_buf, sizeof _buf, __VA_ARGS__);     \
        sb_set_error(obj, _buf);                      \
        return (code);                                \
    } while (0)

#define SB_HIP(obj, call)                                                                       \
    do {                                                                                        \
        hipError_t _r = (call);                                                                 \
        if (_r != hipSuccess) {                                                                 \
            (void)hipGetLastError(); /* reported here: must not resurface in a later launch check */ \
            SB_FAIL(obj, _r == hipErrorOutOfMemory ? SB_ERR_OOM : SB_ERR_HIP, "%s failed: %s",  \
                    #call, hipGetErrorString(_r));                                              \
        }                                                                                       \
    } while (0)

#define SB_TRY(x) do { sb_status _s = (x); if (_s != SB_OK) return _s; } while (0)
