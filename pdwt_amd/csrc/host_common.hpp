// host_common.hpp -- what every host source of libpdwt.so / libpdwtd.so needs next to include/pdwt_hip.h: the precision of this build,
// the device guard of the classes, and the line they print when a C-ABI call fails.  Host only: no .hip unit and none of their headers
// includes it.
#pragma once
#include <stdio.h>

#include "../../include/pdwt_hip.h"

// SFX(pdwt_x) is the entry point of this build's precision, filters_t its bank
#ifndef DOUBLEPRECISION
#define SFX(name) name##_f32
typedef pdwt_filters_f32 filters_t;
#else
#define SFX(name) name##_f64
typedef pdwt_filters_f64 filters_t;
#endif

// Multi-device use from one host thread (the reference has none: TODO.txt:15): an instance belongs to the device that was
// current at its construction; every method that touches device memory switches to that device for its duration, so
// instances on different devices can be driven in turn (their work overlaps: launches are asynchronous).  dev < 0 (an instance
// without private state): nothing to do.
struct DevScope {
    int prev, mine;
    explicit DevScope(int dev) : prev(-1), mine(dev)
    {
        if (mine < 0) return;
        prev = pdwt_get_device();
        if (prev != mine) pdwt_set_device(mine);
    }
    ~DevScope()
    {
        if (mine >= 0 && prev >= 0 && prev != mine) pdwt_set_device(prev);
    }
};

// "ERROR: <class><where> failed ...": where = "::method()" or "(): what"
inline void report(const char* cls, const char* where, int rc) { printf("ERROR: %s%s failed (code %d): %s\n", cls, where, rc, pdwt_last_error_string()); }
