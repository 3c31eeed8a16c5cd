// Probe of the host-side dispatch of the prefill GEMM (csrc/prefill_plan.h) and of the general kernel (vv_gemm_general_plan in
// csrc/gemv_plan.h) for tests/test_prefill_plan_cpu.py: built for the host alone (no device code, no GPU).
// Reads one case per line from stdin, the first word names the plan:
//   g3  T N K ldy epi has_w2 has_y has_yp ws_round g3_bytes   ->  rc form epi n_blocks t_blocks grid.x grid.y block lds full_idx split ks
//   qkv T K D Hq Hkv operands ws_round                         ->  rc (1: fused) and the same plan fields
//   gen xs pro epi T N K ksplit x_misaligned has_w2            ->  rc route vec dual wpb maxr nt ks t_pad grid.x grid.y lds
// Every operand is one dummy address: nothing reads it.
#include <cstdio>
#include <cstring>
#include "gemv_plan.h"
#include "prefill_plan.h"

static void print_plan(int rc, bool valid, const VVGemm3Plan& p) {
    if (!valid) { printf("%d\n", rc); return; }
    printf("%d %d %d %d %d %u %u %d %zu %d %d %d\n", rc, p.form, p.epi, p.n_blocks, p.t_blocks, p.grid.x, p.grid.y, p.block, p.lds, p.full_idx, p.split, p.ks);
}

int main() {
    alignas(16) static char dummy[32];
    char kind[8];
    while (scanf("%7s", kind) == 1) {
        if (!strcmp(kind, "g3")) {
            int T, N, K, ldy, epi, w2, y, yp, round; unsigned long long g3;
            if (scanf("%d %d %d %d %d %d %d %d %d %llu", &T, &N, &K, &ldy, &epi, &w2, &y, &yp, &round, &g3) != 10) return 1;
            VVGemm3Plan p = {};
            const int rc = vv_gemm3_plan(T, N, K, ldy, epi, w2, y, yp, VVPrefillWs{round != 0, (size_t)g3}, &p);
            print_plan(rc, rc == 0, p);
        } else if (!strcmp(kind, "qkv")) {
            int T, K, D, Hq, Hkv, ops, round;
            if (scanf("%d %d %d %d %d %d %d", &T, &K, &D, &Hq, &Hkv, &ops, &round) != 7) return 1;
            VVGemm3Plan p = {};
            const int rc = vv_qkv_rope_plan(T, K, D, Hq, Hkv, ops != 0, round != 0, &p);
            print_plan(rc, rc == 1, p);
        } else if (!strcmp(kind, "gen")) {
            int xs, pro, epi, T, N, K, ksplit, x_mis, w2;
            if (scanf("%d %d %d %d %d %d %d %d %d", &xs, &pro, &epi, &T, &N, &K, &ksplit, &x_mis, &w2) != 9) return 1;
            VVGemm g = {};
            float* const f = (float*)dummy;
            g.W = (const u32x4*)dummy; g.W2 = w2 ? (const u32x4*)dummy : nullptr;
            g.X = (const float*)(dummy + (x_mis ? 4 : 0));
            g.Y = f + 4;
            g.nw = g.mod_scale = g.mod_shift = g.addvec = g.bias = g.gate = f;
            g.T = T; g.N = N; g.K = K; g.ldx = K; g.ldy = N; g.ld_mod = K; g.ld_gate = N;
            g.pro = pro; g.epi = epi; g.ksplit = ksplit; g.nt = 1; g.eps = 1e-6f;
            VVGemmGeneralPlan p = {};
            const int route = vv_gemm_route(&g, xs), rc = vv_gemm_general_plan(&g, xs, &p);
            if (rc != 0) printf("%d %d\n", rc, route);
            else printf("%d %d %d %d %d %d %d %d %d %u %u %zu\n", rc, route, (int)p.vec, (int)p.dual, p.wpb, p.maxr, p.nt, p.ks, p.t_pad, p.grid.x, p.grid.y, p.lds);
        } else return 1;
    }
    return 0;
}
