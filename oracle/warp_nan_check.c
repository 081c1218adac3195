/* Stand-alone check of orc_warp_bilinear's clamps under the address and undefined-behaviour sanitizers (`make -C oracle asan-check`):
 * coordinates that are NaN, +-inf or far outside the image must sample row / column 0 or the last one and read nothing else.  The
 * image sits in a heap block of its exact size, so any read beside it is reported. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include "dfe_oracle.h"

int main(void) {
    static const int sizes[][3] = {{1, 1, 7}, {3, 7, 1}, {5, 5, 6}, {1, 1, 1}};
    const float coords[] = {NAN, -NAN, INFINITY, -INFINITY, -3.5f, 1e30f, -1e30f, 0.f, 0.3f, 2.5f, 4.f, 5.f, 6.f, 16.f};
    const int n = (int)(sizeof(coords) / sizeof(coords[0]));
    int bad = 0;
    for (unsigned s = 0; s < sizeof(sizes) / sizeof(sizes[0]); ++s) {
        const int C = sizes[s][0], H = sizes[s][1], W = sizes[s][2];
        float *img = malloc(sizeof(float) * C * H * W), *mask = malloc(sizeof(float) * 2 * n * n), *out = malloc(sizeof(float) * C * n * n);
        for (int e = 0; e < C * H * W; ++e) img[e] = (float)(e + 1);
        for (int i = 0; i < n; ++i)
            for (int j = 0; j < n; ++j) {
                mask[i * n + j] = coords[i];
                mask[n * n + i * n + j] = coords[j];
            }
        orc_warp_bilinear(img, C, H, W, mask, n, n, out);
        /* NaN in both coordinates samples pixel (0, 0); NaN y with x = +inf the last pixel of row 0 */
        for (int c = 0; c < C; ++c) {
            if (out[c * n * n] != img[c * H * W]) ++bad;
            if (out[c * n * n + 2] != img[c * H * W + W - 1]) ++bad;
            for (int e = 0; e < n * n; ++e)
                if (!(out[c * n * n + e] >= img[c * H * W] && out[c * n * n + e] <= img[(c + 1) * H * W - 1])) ++bad;
        }
        free(img); free(mask); free(out);
    }
    printf("warp_nan_check: %s\n", bad ? "FAILED" : "ok");
    return bad != 0;
}
