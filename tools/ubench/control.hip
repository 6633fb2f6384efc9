// Control-flow and lane-mask bookkeeping costs for a lone gfx950 wavefront: cycles per occurrence of a branch, an exec-mask `if`, a 64-bit
// SALU mask operation, a satisfied s_waitcnt and a v_readlane + s_nop, each set into a stream of independent fp64 v_fma (eight per occurrence)
// and measured as the difference to the same stream without it.  One wave64 per workgroup with 40 KB of LDS, so four workgroups per CU: one
// wavefront on every SIMD, the occupancy of the headline closed-loop kernel; the SIMD ids of the wavefronts are counted and printed.
// build: hipcc -O3 --offload-arch=gfx950 tools/ubench/control.hip -o tools/ubench/control      run: tools/ubench/control [steps-table]
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define HIPCHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); exit(1); } } while (0)

#define R4(x) x x x x
#define R16(x) R4(x) R4(x) R4(x) R4(x)
// 16 groups per pass of a loop that is not unrolled: at most 3.5 KB of code, resident in the instruction cache after the first pass
constexpr int kIters = 256, kGroups = 16;

// filler: independent fp64 fma on four accumulators
#define F4 "v_fma_f64 %0, %0, %4, %5\n v_fma_f64 %1, %1, %4, %5\n v_fma_f64 %2, %2, %4, %5\n v_fma_f64 %3, %3, %4, %5\n"
#define F8 F4 F4
#define F16 F8 F8

#define KERNEL(NAME, BODY, ...)                                                                          \
    __global__ __launch_bounds__(64) void NAME(double *out, unsigned long long *cyc, unsigned *simd, double seed) { \
        double a0 = seed + threadIdx.x, a1 = a0 + 1, a2 = a0 + 2, a3 = a0 + 3, b = 1.0000001, c = 1e-9;     \
        int i0 = threadIdx.x;                                                                            \
        __shared__ double lds[5000];                           /* 40 000 bytes: four workgroups per CU */ \
        lds[threadIdx.x] = a0;                                                                           \
        for (int j = threadIdx.x + 64; j < 5000; j += 64 * 13) lds[j] = a1;                              \
        asm volatile("s_mov_b64 s[20:21], exec\n s_mov_b64 s[22:23], 0\n s_mov_b32 s24, 0xaaaaaaaa\n s_mov_b32 s25, 0xaaaaaaaa"        \
                     ::: "s20", "s21", "s22", "s23", "s24", "s25");                                      \
        __syncthreads();                                                                                 \
        unsigned long long t0 = __builtin_amdgcn_s_memtime();                                            \
        __builtin_amdgcn_s_waitcnt(0xC07F);                                                              \
        _Pragma("unroll 1")                                                                              \
        for (int it = 0; it < kIters; ++it) {                                                            \
            asm volatile(R16(BODY) : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3) : "v"(b), "v"(c), "v"(i0) : __VA_ARGS__); \
        }                                                                                                \
        unsigned long long t1 = __builtin_amdgcn_s_memtime();                                            \
        __builtin_amdgcn_s_waitcnt(0xC07F);                                                              \
        out[blockIdx.x * 64 + threadIdx.x] = a0 + a1 + a2 + a3 + lds[(threadIdx.x * 77) % 5000];         \
        if (threadIdx.x == 0) {                                                                          \
            unsigned hw;                                                                                 \
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));                              \
            cyc[blockIdx.x] = t1 - t0;                                                                   \
            simd[blockIdx.x] = (hw >> 4) & 3u;                                                           \
        }                                                                                                \
    }

// operands: %0-%3 doubles a0..a3 (all > 1), %4 b, %5 c (1e-9), %6 an int; s[20:21] = exec at entry, s[22:23] scratch mask
KERNEL(k_base8, F8, "memory")
KERNEL(k_base10, F8 "v_fma_f64 %0, %0, %4, %5\n v_fma_f64 %1, %1, %4, %5\n", "memory")
// exec is never zero here: execnz is always taken, execz never.  The taken branch jumps over 16 fma (128 bytes) into another 64-byte line.
KERNEL(k_br_taken, "s_cbranch_execnz 1f\n" F16 "1:\n" F8, "memory")
KERNEL(k_br_taken_near, "s_cbranch_execnz 1f\n v_fma_f64 %0, %0, %4, %5\n 1:\n" F8, "memory")
KERNEL(k_br_not_taken, "s_cbranch_execz 1f\n" F8 "1:\n", "memory")
// the compiler's `if (lane condition) { two instructions }`: a0 > c holds on every lane, a0 < c on none
KERNEL(k_if_entered, "v_cmp_gt_f64 vcc, %0, %5\n s_and_saveexec_b64 s[22:23], vcc\n s_cbranch_execz 1f\n v_fma_f64 %0, %0, %4, %5\n v_fma_f64 %1, %1, %4, %5\n"
                     "1:\n s_or_b64 exec, exec, s[22:23]\n" F8, "memory", "vcc", "s22", "s23")
KERNEL(k_if_skipped, "v_cmp_lt_f64 vcc, %0, %5\n s_and_saveexec_b64 s[22:23], vcc\n s_cbranch_execz 1f\n v_fma_f64 %0, %0, %4, %5\n v_fma_f64 %1, %1, %4, %5\n"
                     "1:\n s_or_b64 exec, exec, s[22:23]\n" F8, "memory", "vcc", "s22", "s23")
KERNEL(k_if_skipped_far, "v_cmp_lt_f64 vcc, %0, %5\n s_and_saveexec_b64 s[22:23], vcc\n s_cbranch_execz 1f\n" F16
                         "1:\n s_or_b64 exec, exec, s[22:23]\n" F8, "memory", "vcc", "s22", "s23")
// the same `if` as a select: compare, the two fma, two 64-bit selects (four v_cndmask, on registers of their own: only the issue slots count)
KERNEL(k_if_select, "v_cmp_gt_f64 vcc, %0, %5\n v_fma_f64 %0, %0, %4, %5\n v_fma_f64 %1, %1, %4, %5\n"
                    "v_cndmask_b32 v200, v200, v201, vcc\n v_cndmask_b32 v202, v202, v203, vcc\n v_cndmask_b32 v201, v201, v200, vcc\n v_cndmask_b32 v203, v203, v202, vcc\n" F8,
       "memory", "vcc", "v200", "v201", "v202", "v203")
// a per-lane choice between two doubles by lane parity, as the compiler writes `odd ? pinned(a) : pinned(b)` with the pin (an empty volatile asm)
// inside the arms -- two exec regions, the second entered by a taken branch, a 64-bit move in it -- and as two v_cndmask
KERNEL(k_choice_regions, "s_and_saveexec_b64 s[22:23], s[24:25]\n s_xor_b64 s[22:23], exec, s[22:23]\n s_cbranch_execz 1f\n"
                         "s_andn2_saveexec_b64 s[22:23], s[22:23]\n s_cbranch_execnz 2f\n 1:\n" F16
                         "2:\n s_nop 0\n v_mov_b64 v[200:201], v[202:203]\n s_or_b64 exec, exec, s[22:23]\n" F8, "memory", "scc", "s22", "s23", "v200", "v201")
KERNEL(k_choice_select, "v_cndmask_b32 v200, v200, v202, s[24:25]\n v_cndmask_b32 v201, v201, v203, s[24:25]\n" F8, "memory", "v200", "v201")
KERNEL(k_mask_op, F4 "s_or_b64 s[22:23], s[22:23], s[20:21]\n" F4, "memory", "scc", "s22", "s23")
KERNEL(k_mask_op_of_cmp, F4 "v_cmp_gt_f64 vcc, %0, %5\n s_and_b64 s[22:23], vcc, s[20:21]\n" F4, "memory", "scc", "vcc", "s22", "s23")
KERNEL(k_cmp_only, F4 "v_cmp_gt_f64 vcc, %0, %5\n" F4, "memory", "vcc")
KERNEL(k_waitcnt, F4 "s_waitcnt vmcnt(0) lgkmcnt(0)\n" F4, "memory")
KERNEL(k_readlane_nop, F4 "v_readlane_b32 s22, %6, 3\n s_nop 0\n" F4, "memory", "s22")
KERNEL(k_readlane, F4 "v_readlane_b32 s22, %6, 3\n" F4, "memory", "s22")

typedef void (*kern_t)(double *, unsigned long long *, unsigned *, double);
struct Entry { const char *name; kern_t fn; int base; double per_step; };      // base: index of the kernel whose time is subtracted (-1: none)

int main(int argc, char **argv) {
    setvbuf(stdout, NULL, _IONBF, 0);
    // occurrences per executed step of the headline kernel (static count of the plain step, DESIGN_APPENDIX): 0 = not applicable
    Entry tab[] = {
        {"8 v_fma_f64 (filler, per group)", k_base8, -1, 0},
        {"10 v_fma_f64 (filler + body of the `if`)", k_base10, -1, 0},
        {"s_cbranch taken, target in another 64-byte line", k_br_taken, 0, 7},
        {"s_cbranch taken, target one instruction ahead", k_br_taken_near, 0, 0},
        {"s_cbranch not taken", k_br_not_taken, 0, 7},
        {"v_cmp + s_and_saveexec + s_cbranch_execz + s_or exec, entered", k_if_entered, 1, 7},
        {"v_cmp + s_and_saveexec + s_cbranch_execz + s_or exec, skipped", k_if_skipped, 0, 0},
        {"  the same, skipping 16 instructions", k_if_skipped_far, 0, 0},
        {"  the entered `if` as v_cmp + 2 fma + 2 v_cndmask", k_if_select, 1, 0},
        {"v_cmp_gt_f64 alone", k_cmp_only, 0, 0},
        {"choice of a double by lane parity: two exec regions, one taken branch", k_choice_regions, 0, 6},
        {"choice of a double by lane parity: two v_cndmask_b32", k_choice_select, 0, 0},
        {"s_or_b64 between VALU instructions", k_mask_op, 0, 75},
        {"v_cmp + s_and_b64 of its result", k_mask_op_of_cmp, 0, 0},
        {"s_waitcnt, already satisfied", k_waitcnt, 0, 34},
        {"v_readlane_b32 + s_nop 0", k_readlane_nop, 0, 8},
        {"v_readlane_b32 alone", k_readlane, 0, 0},
    };
    const int n = sizeof(tab) / sizeof(tab[0]);
    const int blocks = 1024;                                   // 256 CUs x 4 SIMDs
    const double step_cycles = 9100.0;
    double *out; unsigned long long *cyc; unsigned *simd;
    HIPCHECK(hipMalloc(&out, (size_t)blocks * 64 * sizeof(double)));
    HIPCHECK(hipMalloc(&cyc, blocks * sizeof(unsigned long long)));
    HIPCHECK(hipMalloc(&simd, blocks * sizeof(unsigned)));
    std::vector<double> per_group(n);
    printf("%d single-wave workgroups, 40 KB LDS each; s_memtime cycles per group of 8 filler fma + one occurrence, mean over wavefronts\n", blocks);
    printf("%-66s %9s %9s %9s %8s %8s\n", "pattern", "cyc/grp", "min", "max", "delta", "simd0-3");
    for (int i = 0; i < n; ++i) {
        for (int w = 0; w < 2; ++w) hipLaunchKernelGGL(tab[i].fn, dim3(blocks), dim3(64), 0, 0, out, cyc, simd, 1.5);
        HIPCHECK(hipDeviceSynchronize());
        std::vector<unsigned long long> h(blocks);
        std::vector<unsigned> sd(blocks);
        HIPCHECK(hipMemcpy(h.data(), cyc, blocks * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        HIPCHECK(hipMemcpy(sd.data(), simd, blocks * sizeof(unsigned), hipMemcpyDeviceToHost));
        double s = 0, lo = 1e30, hi = 0;
        int cnt[4] = {0, 0, 0, 0};
        for (int b = 0; b < blocks; ++b) {
            const double v = (double)h[b] / (kIters * kGroups);
            s += v; lo = v < lo ? v : lo; hi = v > hi ? v : hi;
            cnt[sd[b] & 3]++;
        }
        per_group[i] = s / blocks;
        char delta[32] = "";
        if (tab[i].base >= 0) snprintf(delta, sizeof delta, "%8.2f", per_group[i] - per_group[tab[i].base]);
        printf("%-66s %9.2f %9.2f %9.2f %8s %d/%d/%d/%d\n", tab[i].name, per_group[i], lo, hi, delta, cnt[0], cnt[1], cnt[2], cnt[3]);
    }
    // an s_memtime tick is a shader cycle: the deltas are cycles per occurrence; the filler line is the check against tools/ubench/issue.hip
    printf("\nfiller: %.2f cycles per independent v_fma_f64.  Count per executed step x cost, against the %.0f-cycle step:\n", per_group[0] / 8.0, step_cycles);
    printf("%-66s %8s %10s %12s %9s\n", "class", "cycles", "per step", "cycles/step", "% of step");
    for (int i = 0; i < n; ++i) {
        if (tab[i].base < 0) continue;
        const double c = per_group[i] - per_group[tab[i].base];
        if (tab[i].per_step > 0)
            printf("%-66s %8.2f %10.0f %12.1f %8.2f%%\n", tab[i].name, c, tab[i].per_step, c * tab[i].per_step, 100.0 * c * tab[i].per_step / step_cycles);
        else
            printf("%-66s %8.2f\n", tab[i].name, c);
    }
    HIPCHECK(hipFree(out)); HIPCHECK(hipFree(cyc)); HIPCHECK(hipFree(simd));
    return 0;
}
