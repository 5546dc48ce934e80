// cubic.h -- the Catmull-Rom cubic through four equally spaced samples p0..p3, evaluated at x in [0, 1) between p1 and p2: the
// arithmetic of image.scale(.., 'bicubic') (kernels_scale.hip) and of the equirectangular gather (kernels_equi.hip).  Both units are
// compiled with -ffp-contract=off, so every operation rounds as written (tests/util/bicubic_model.py, tests/util/equi_model.py).
#pragma once
#include <hip/hip_runtime.h>

namespace fav {

__device__ __forceinline__ float catmull_rom(float p0, float p1, float p2, float p3, float x)
{
    const float a1 = p2 - p0;
    const float a2 = 2.f * p0 - 5.f * p1 + 4.f * p2 - p3;
    const float a3 = 3.f * (p1 - p2) + p3 - p0;
    return p1 + 0.5f * x * (a1 + x * (a2 + x * a3));
}

}  // namespace fav
