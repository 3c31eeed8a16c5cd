"""The (T, N, K) lists of the prefill GEMM's GPU tests and the engine settings that decide their workspace, as plain tuples: the GPU
tests parametrise over them, and test_prefill_plan_cpu.py asks the dispatch (csrc/prefill_plan.h), on a machine without a GPU,
whether every shape runs the kernel its test says it does."""

# test_gpu_kernels.py::test_prefill_gemm3: the last PREFILL_GEMM3_ON_G4 shapes fill the chip with 256 x 256 workgroups
# (vv_gemm4_kernel), the others run vv_gemm3_kernel.  Its engine has no K-split workspace (exact mode).
PREFILL_GEMM3 = [(333, 4112, 416), (128, 128, 64), (2048, 1024, 1536), (70, 200, 96), (500, 36, 3584), (4100, 4112, 416), (4100, 4100, 2080)]
PREFILL_GEMM3_ON_G4 = 2
PREFILL_GEMM3_EPIS = [0, 1, 4, 3]

# test_gpu_shipped.py::test_prefill_gemm4_k_split_round: every shape, under every epilogue, splits the partial round of vv_gemm4_kernel
K_SPLIT_ROUND = [(4100, 4112, 2080), (4352, 4096, 2048), (2100, 7420, 1568)]
K_SPLIT_ROUND_EPIS = [0, 1, 4, 3]
K_SPLIT_ROUND_ENGINE = ("0.5b", 1024)           # (geometry of test_gpu_geometry.GEOM, max_rows), bf16-activation mode

# test_gpu_shipped.py::test_short_prompt_gemm3_k_split_and_reduce: every shape splits K over grid.y of the double-buffered vv_gemm3_kernel
SHORT_PROMPT = [(330, 1536, 8960), (330, 2048, 1536), (333, 1540, 1056), (75, 896, 4864), (500, 36, 3584)]
SHORT_PROMPT_EPIS = [0, 1, 4]
SHORT_PROMPT_ENGINE = ("0.5b", 512)
