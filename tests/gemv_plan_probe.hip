// Probe of the host-side GEMM dispatch for tests/test_gemv_plan_cpu.py: built for the host alone (no device code, no GPU).
// Reads one case per line from stdin:
//   xs pro epi T N K kgrid n_xa n_ya sl_n sl_T ksplit n_cfg x_row_mod x_misaligned
// and prints  eligible has_form  xs mr wpb parts sl  grid.x grid.y  route.  Every operand is one dummy address: nothing reads it.
#include <cstdio>
#include "gemv_plan.h"

int main() {
    alignas(16) static char dummy[32];
    int xs, pro, epi, T, N, K, kgrid, n_xa, n_ya, sl_n, sl_T, ksplit, n_cfg, x_row_mod, x_mis;
    while (scanf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d", &xs, &pro, &epi, &T, &N, &K, &kgrid, &n_xa, &n_ya, &sl_n, &sl_T, &ksplit, &n_cfg,
                 &x_row_mod, &x_mis) == 15) {
        VVGemm g = {};
        float* const p = (float*)dummy;
        g.W = g.W2 = (const u32x4*)dummy;
        g.X = (const float*)(dummy + (x_mis ? 4 : 0));
        g.Y = g.z = g.x0p = g.yparts = g.dw_xout = p + 4;      // dw_xout must differ from X
        g.dw_hnew = p;
        g.nw = g.mod_scale = g.mod_shift = g.addvec = g.bias = g.gate = g.coef = g.xa = g.ya = p;
        g.dw_hist = g.dw_w = g.dw_b = g.dw_gamma = g.dw_nw = p;
        g.T = T; g.N = N; g.K = K; g.ldx = K; g.ldy = N; g.ld_mod = K; g.ld_gate = N;
        g.pro = pro; g.epi = epi; g.ksplit = ksplit; g.nt = 1; g.n_cfg = n_cfg; g.x_row_mod = x_row_mod; g.eps = 1e-6f;
        g.kgrid = kgrid; g.n_xa = n_xa; g.n_ya = n_ya; g.part_stride = n_xa ? T * K : T * N;
        g.sl_n = sl_n; g.sl_T = sl_T; g.sl_x = sl_T * K; g.sl_y = sl_T * N;
        for (int j = 0; j < 8; ++j) g.sl_id[j] = j < sl_n ? j : 0;
        VVGemvPlan plan = {};
        const bool has = vv_gemv_plan(&g, xs, &plan);
        printf("%d %d  %d %d %d %d %d  %u %u  %d\n", (int)vv_gemv_eligible(&g), (int)has, plan.form.xs, plan.form.mr, plan.form.wpb, plan.form.parts,
               plan.form.sl, has ? plan.grid.x : 0u, has ? plan.grid.y : 0u, vv_gemm_route(&g, xs));
    }
    return 0;
}
