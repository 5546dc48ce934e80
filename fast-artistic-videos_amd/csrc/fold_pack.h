// fold_pack.h -- host-side weight packing for the row-folded last layer (c9s1-3: few output channels, the kx taps folded into N;
// kernels_fold.hip).  Plain C++ (no HIP): the CPU test suite compiles it on its own.
#pragma once
#include <cstddef>
#include <vector>

namespace fav {

// w: [cout][cin][k][k]; cinp: the channel pitch of the input (cin <= cinp), cout * k <= 32 (conv_fold_eligible)
inline void conv_fold_pack(const float* w, int cin, int cinp, int cout, int k, std::vector<float>& out)
{
    // [ky][n = c*k + kx][ci] for the row-folded last-layer kernel
    // followed by the K+1 merged slices Wm[m] = W[m-1] + W[m] (W[-1] = W[K] = 0) for a x2-upsampled input
    // (conv_rowfold_up2_kernel: the logical rows 2r and 2r+1 are the same physical row)
    out.assign((size_t)(2 * k + 1) * 32 * cinp, 0.f);
    for (int co = 0; co < cout; ++co)
        for (int ci = 0; ci < cin; ++ci)
            for (int ky = 0; ky < k; ++ky)
                for (int kx = 0; kx < k; ++kx)
                    out[((size_t)ky * 32 + co * k + kx) * cinp + ci] = w[(((size_t)co * cin + ci) * k + ky) * k + kx];
    for (int co = 0; co < cout; ++co)
        for (int ci = 0; ci < cin; ++ci)
            for (int m = 0; m <= k; ++m)
                for (int kx = 0; kx < k; ++kx) {
                    const float* wr = &w[((size_t)co * cin + ci) * k * k + kx];
                    const double a = m >= 1 ? (double)wr[(size_t)(m - 1) * k] : 0.0, b = m < k ? (double)wr[(size_t)m * k] : 0.0;
                    out[((size_t)(k + m) * 32 + co * k + kx) * cinp + ci] = (float)(a + b);
                }
}

}  // namespace fav
