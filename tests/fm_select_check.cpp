// fm_select_check.cpp -- a host program over csrc/fm_select.h, built and run by tests/test_fm_select_cpu.py under ASan / UBSan.
// With cases on stdin -- one per line, 20 integers:
//   cv_mode fm_flat fm64 fm_rows fm_mfma fm_split  form K H1 W1 maxh maxw pitch1 plane1  in1 in2 out (addresses: only their low bits count)
//   soft_full hFull wFull (FM_SOFT / FM_MEAN: whether the full-frame planes are asked for, and their size)
// it prints one line per case: the name dfe_last_kernel would report ("none" for FM_K_NONE) and, for the flat tiles, S, nd and LDS bytes.
// With no input it sweeps the shapes around every guard, checks what must hold for every pick, and prints the largest flat-tile LDS size
// and "ok".  The first failed check prints its line and exits 1.
#include "fm_select.h"
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

#define CHECK(c) do { if (!(c)) { printf("fm_select_check.cpp:%d: %s\n", __LINE__, #c); exit(1); } } while (0)

static int sweep() {
    static float out_plane[1];
    size_t flat_max = 0;
    long long picks[FM_K_REF + 1] = {};
    for (int cv = 0; cv <= 2; ++cv)
    for (int mfma = 0; mfma <= 1; ++mfma)
    for (int form = FM_VOLUME; form <= FM_MEAN; ++form)
    for (int maxh = 1; maxh <= 20; ++maxh)
    for (int maxw = 1; maxw <= 20; ++maxw)
    for (int K : {1, 8, 16, 17, 256, 257})
    for (int W1 : {1, 7, 8, 252, 253, 400, 625})
    for (int H1 : {1, 7, 8, 16, 465}) {
        const FmEnv e{cv, -1, -1, -1, mfma, -1};
        DfeSoftOut so{};
        so.hFull = H1 + maxh - 1; so.wFull = W1 + maxw - 1; so.full = out_plane;
        FmJob j = fm_job((FmForm)form, nullptr, nullptr, K, H1, W1, maxh, maxw);
        if (form == FM_VOLUME) j.out = (float *)(uintptr_t)256;
        if (form >= FM_SOFT) j.soft = &so;
        const FmPick p = fm_select(e, j);
        ++picks[p.kernel];
        if (form == FM_VOLUME) CHECK(p.kernel != FM_K_NONE);                       // the volume of contiguous maps always has a kernel
        else CHECK(p.kernel == FM_K_MFMA || p.kernel == FM_K_FLAT || p.kernel == FM_K_NONE);
        if (cv == 1) CHECK(p.kernel == FM_K_REF || p.kernel == FM_K_NONE);
        if (!mfma) CHECK(p.kernel != FM_K_MFMA);
        if (p.kernel == FM_K_FLAT) {
            CHECK(p.lds * p.S <= 160 * 1024 && p.S >= 1 && p.nd >= 1 && p.nd <= 16);
            if (p.lds > flat_max) flat_max = p.lds;
        }
        if (p.kernel == FM_K_WIN64) CHECK(p.lds <= 64 * 1024 && p.pitch >= FM_TX + maxw - 1);
        if (p.kernel == FM_K_CHUNK) CHECK(p.KB >= 1 && p.KB <= K && p.lds <= 48 * 1024);
        if (p.kernel == FM_K_MFMA) CHECK((p.KC == 8 || p.KC == 16) && p.lds <= 160 * 1024);
        // the same maps as a view with padded rows: only the flat tiles read one, and they take it wherever they take the contiguous maps
        const bool flat_takes = fm_select(FmEnv{cv, -1, -1, -1, 0, -1}, j).kernel == FM_K_FLAT;
        j.pitch1 = W1 + 3; j.plane1 = (long long)H1 * j.pitch1 + 5;
        const FmPick v = fm_select(e, j);
        CHECK(v.kernel == (flat_takes ? FM_K_FLAT : FM_K_NONE));
    }
    for (int k = FM_K_MFMA; k <= FM_K_REF; ++k) CHECK(picks[k] > 0);               // the sweep reaches every family
    printf("flat_lds_max %zu\nok\n", flat_max);
    return 0;
}

int main() {
    static float plane[1];
    long long v[20];
    int ncases = 0;
    for (;;) {
        int n = 0;
        while (n < 20 && scanf("%lld", &v[n]) == 1) ++n;
        if (n == 0) break;
        CHECK(n == 20);
        ++ncases;
        const FmEnv e{(int)v[0], (int)v[1], (int)v[2], (int)v[3], (int)v[4], (int)v[5]};
        FmJob j = fm_job((FmForm)v[6], (const float *)(uintptr_t)v[14], (const float *)(uintptr_t)v[15], (int)v[7], (int)v[8], (int)v[9], (int)v[10], (int)v[11]);
        j.pitch1 = (int)v[12]; j.plane1 = v[13];
        j.out = (float *)(uintptr_t)v[16];
        DfeSoftOut so{};
        so.full = v[17] ? plane : nullptr; so.hFull = (int)v[18]; so.wFull = (int)v[19];
        if (j.form >= FM_SOFT) j.soft = &so;
        const FmPick p = fm_select(e, j);
        if (p.kernel == FM_K_NONE) puts("none");
        else if (p.kernel == FM_K_FLAT) printf("%s %d %d %zu\n", fm_kernel_name(p.kernel, j.form), p.S, p.nd, p.lds);
        else puts(fm_kernel_name(p.kernel, j.form));
    }
    return ncases ? 0 : sweep();
}
