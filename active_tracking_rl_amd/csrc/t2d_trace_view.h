// t2d_trace_view.h — the one internal seam between csrc/track2d_hip.hip (which owns t2d_handle) and csrc/render_hip.hip
// (episode traces + renderer, include/track2d_trace.h): the device arrays the renderer reads and the slot through which the
// handle owns the trace store. Not part of the public ABI.
#pragma once
#include <stdint.h>

#include "../../include/track2d.h"

struct t2d_trace_view {
    int device, n, auto_reset;
    const uint32_t *maps;   // [N][256] bit-packed tiles (t2d_device.h)
    const uint32_t *pos;    // [N] tracker r | c<<8 | target r<<16 | c<<24
    const uint32_t *cnt;    // [N] c_far | t<<8 | side<<24
    uint32_t *faults;       // [1] sticky fault word
    void **store;           // the handle's trace-store slot and its destructor: t2d_destroy calls (*store_free)(*store)
    void (**store_free)(void *);
};

extern "C" int t2d_trace_view_get(t2d_handle *h, t2d_trace_view *out);
