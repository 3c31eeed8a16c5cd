// Probe of the W13 side of the host dispatch for tests/test_w13_plan_cpu.py: built for the host alone (no device code, no GPU).
// Reads one case per line from stdin, the first word names the question:
//   form xs pro epi T N K kgrid n_xa      ->  vv_gemv_w13_form  mr wpb   (mr, wpb of the form; 0 0 where the answer is -1)
//   lm   w13 tile3_ok attn2_ok p16_ok n_rows (cache pos) x n_rows      ->  rc route w13
// Every operand is one dummy address: nothing reads it.
#include <cstdio>
#include <cstring>
#include <vector>
#include "gemv_plan.h"
#include "pass_plan.h"

int main() {
    alignas(16) static char dummy[32];
    char kind[8];
    while (scanf("%7s", kind) == 1) {
        if (!strcmp(kind, "form")) {
            int xs, pro, epi, T, N, K, kgrid, n_xa;
            if (scanf("%d %d %d %d %d %d %d %d", &xs, &pro, &epi, &T, &N, &K, &kgrid, &n_xa) != 8) return 1;
            VVGemm g = {};
            float* const p = (float*)dummy;
            g.W = g.W2 = (const u32x4*)dummy;
            g.X = p; g.Y = g.yparts = p + 4;
            g.nw = g.bias = g.xa = p;
            g.T = T; g.N = N; g.K = K; g.ldx = K; g.ldy = N;
            g.pro = pro; g.epi = epi; g.nt = 1; g.eps = 1e-6f;
            g.kgrid = kgrid; g.n_xa = n_xa; g.part_stride = n_xa ? T * K : T * N;
            const int f = vv_gemv_w13_form(&g, xs);
            printf("%d %d %d\n", f, f >= 0 ? vv_gemv_w13_forms[f].mr : 0, f >= 0 ? vv_gemv_w13_forms[f].wpb : 0);
        } else if (!strcmp(kind, "lm")) {
            int w13, t3, a2, p16, n;
            if (scanf("%d %d %d %d %d", &w13, &t3, &a2, &p16, &n) != 5 || n < 1) return 1;
            std::vector<VVRow> rows(n);
            for (auto& r : rows) if (scanf("%d %d", &r.cache, &r.pos) != 2) return 1;
            VVLmCaps caps{64, 128, 2, t3 != 0, a2 != 0, p16 != 0};
            caps.w13 = w13 != 0;
            VVLmPlan p = {};
            const int rc = vv_lm_pass_plan(rows.data(), n, caps, &p);
            printf("%d %d %d\n", rc, rc ? -1 : p.route, rc ? 0 : (int)p.w13);
        } else return 1;
    }
    return 0;
}
