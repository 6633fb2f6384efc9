// Diagnostic clocks and phase stamps of the tuned kernels (rmckf_tuned.hpp, rmckf_wide.hpp): compile-time switches, dead code in the shipped library.
#pragma once
#include "rmckf_device.hpp"

namespace uvs {

// ---- Diagnostic builds (`make stamps`, `make quick QDEF=-DUVS_...`; into tools/diag/, never the shipped library).  One switch each; the
// kernel below reads them with `if constexpr`, so a build without them contains none of this code.  Each writes its clock sums over the first
// words of a wavefront's / segment's slice of `stats` (garbage in that build) and is read with tools/read_stamps.py / tools/wave_times.py:
//   UVS_STAMPS       per-phase cycle sums (s_memtime) of the step loop            UVS_FPI_STAMPS   cycles of the MCKF fixed-point branch by phase
//   UVS_ITEM_STAMPS  where a work item's time goes (entry / state / steps / hand-over, 100 MHz clock)
//   UVS_WAVE_TIMES   when and where every wavefront ran (100 MHz clock, HW_ID, XCC_ID)
#ifdef UVS_STAMPS
constexpr bool kDiagStamps = true;
#else
constexpr bool kDiagStamps = false;
#endif
#ifdef UVS_FPI_STAMPS
constexpr bool kDiagFpi = true;
#else
constexpr bool kDiagFpi = false;
#endif
#ifdef UVS_ITEM_STAMPS
constexpr bool kDiagItems = true;
#else
constexpr bool kDiagItems = false;
#endif
#ifdef UVS_WAVE_TIMES
constexpr bool kDiagWaves = true;
#else
constexpr bool kDiagWaves = false;
#endif

UVS_DEV unsigned long long diag_cycles() {                       // shader clock
    unsigned long long t;
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
    return t;
}
UVS_DEV unsigned long long diag_ticks() {                        // constant 100 MHz clock, one for the whole device
    unsigned long long t;
    asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
    return t;
}
struct DiagPhases {                                              // sums of cycles between consecutive stamps, by slot
    unsigned long long sum[8] = {0, 0, 0, 0, 0, 0, 0, 0}, last = 0;
    UVS_DEV void stamp(int slot) {                               // slot < 0: restart the interval without booking it
        __builtin_amdgcn_sched_barrier(0);
        const unsigned long long now = diag_cycles();
        __builtin_amdgcn_sched_barrier(0);
        if (slot >= 0) sum[slot] += now - last;
        last = now;
    }
};
#define UVS_STAMP(slot) do { if constexpr (kDiagStamps) diag_steps.stamp(slot); } while (0)
#define UVS_FPI_STAMP(slot) do { if constexpr (kDiagFpi) diag_fpi.stamp(slot); } while (0)

}  // namespace uvs
