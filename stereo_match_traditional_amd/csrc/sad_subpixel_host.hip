// smt_sad_subpixel_host: the maps of smt_sad_subpixel / smt_sad_both_subpixel on host buffers with no GPU -- the loops of
// GetPointDepthLeft and GetPointDepthRight (Sad.h:96-182) written out, the selection and the parabola through the rule
// header the kernels include (csrc/sad_subpixel_rule.h).  The subject of tests/test_sad_subpixel_cpu.py.
#include "smt_common.h"
#include "sad_subpixel_rule.h"
#include "../../include/smt_sad_subpixel.h"
#include <stdlib.h>
#include <vector>

SMT_API int smt_sad_subpixel_host(const uint8_t *Lp, const uint8_t *Rp, int H, int W, int D, int winsize,
                                  const smt_subpixel_params *params, float *dispL, float *dispR, int32_t *winL, int32_t *winR)
{
    if (!Lp || !Rp || H <= 0 || W <= 0 || D <= 0 || D > SMT_MAX_DISPARITY || winsize < 0) return SMT_ERR_ARG;
    const float md = params ? params->min_den : 1.0f;
    if (!spx_min_den_ok(md)) return SMT_ERR_ARG;
    const int w = winsize + 1, side = 2 * w + 1;
    const size_t Wp = (size_t)W + 2 * (size_t)w;
    // sadvalue (:15-20) of the left window at column xl against the right window at column xr, both in row i
    auto cost = [&](int i, int xl, int xr) {
        unsigned acc = 0;
        for (int r = 0; r < side; r++)
            for (int c = 0; c < side; c++)
                acc += (unsigned)abs((int)Lp[(size_t)(i + r) * Wp + xl + c] - (int)Rp[(size_t)(i + r) * Wp + xr + c]);
        return (float)acc;
    };
    std::vector<float> sad(D);
    for (int i = 0; i < H; i++)
        for (int x = 0; x < W; x++) {
            const size_t p = (size_t)i * W + x;
            if (dispL || winL) {
                for (int d = 0; d < D; d++) sad[d] = d <= x ? cost(i, x, x - d) : sad[d - 1];        // :125-131
                const int r = sad_optimal_row(sad.data(), D);
                if (winL) winL[p] = r;
                if (dispL) dispL[p] = sad_spx_row(r, sad.data(), D, md);
            }
            if (dispR || winR) {
                int wd = 0;
                float f = 0.0f;                                                                     // :157, :160
                if (i < H - 1 && x < W - 1) {
                    for (int d = 0; d < D; d++) sad[d] = x + d <= W - 1 ? cost(i, x + d, x) : sad[d - 1];   // :167-174
                    wd = spx_winner(sad.data(), D);                                                 // GetMinSadIndex :22-38
                    f = sad_spx_row(wd, sad.data(), D, md);
                }
                if (winR) winR[p] = wd;
                if (dispR) dispR[p] = f;
            }
        }
    return SMT_OK;
}
