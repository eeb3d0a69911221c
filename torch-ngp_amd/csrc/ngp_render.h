// The device-driven render loop's state record, shared by raymarching.hip
// (the loop's kernels) and frame.hip (the frame renderer's begin kernel, which
// initialises it). Header-only.
#pragma once
#include <stdint.h>

namespace ngp_render {

// One of the two slots of the loop state: iteration i reads slot i & 1 and
// prepares slot (i + 1) & 1.
struct RenderSlot {
    int32_t count;    // samples this iteration: n_alive * n_step (0 once done); the grid / MLP count
    int32_t n_alive;  // rays in this iteration's alive list
    int32_t step;     // the reference's `step` before this iteration
    int32_t pad;
};

}  // namespace ngp_render
