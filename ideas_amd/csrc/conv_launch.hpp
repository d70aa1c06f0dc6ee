// Host-side launch rules shared by the convolution families: flag dispatch, environment switches, extents, the device query and
// the pieces of split-K sizing.  No device code.  DESIGN.md §3.1.1 lists which site combines the pieces how.
#pragma once
#include <stdlib.h>
#include <algorithm>
#include <type_traits>
#include "common.hpp"

// f(std::integral_constant<bool, a>, std::integral_constant<bool, b>): two run-time flags as template arguments
template <typename F> static inline void with_flags(bool a, bool b, F&& f) {
    if (a) { if (b) f(std::true_type{}, std::true_type{}); else f(std::true_type{}, std::false_type{}); }
    else { if (b) f(std::false_type{}, std::true_type{}); else f(std::false_type{}, std::false_type{}); }
}
// an A/B switch of the environment set to "0" (read per call: no state in the library, include/ideas_hip.h)
static inline bool ideas_env_off(const char* name) { const char* e = getenv(name); return e && e[0] == '0'; }

// byte extent of an NHWC tensor as the `unsigned` of a raw buffer resource (the *_supported rules keep it below 2^32)
static inline unsigned ideas_nhwc_bytes(int B, int H, int W, int C, int elt) { return (unsigned)((int64_t)B * H * W * C * elt); }
static inline unsigned ideas_x_bytes(const ideas_conv_params* p, int elt) { return ideas_nhwc_bytes(p->B, p->IH, p->IW, p->Cin, elt); }
static inline unsigned ideas_gy_bytes(const ideas_conv_params* p, int elt) { return ideas_nhwc_bytes(p->B, p->YH, p->YW, p->Cout, elt); }
static inline bool ideas_grid_fits(int64_t blocks) { return blocks <= 0x7fffffffLL; }      // a 1-D grid

// ---- device query: what include/ideas_hip.h allows to be memoised per process, initialised once and thread-safely ---------------
inline int ideas_cu_count() {                                  // (inline, not static: ONE value for the whole library)
    static const int n = [] {
        int dev = 0;
        hipDeviceProp_t prop;
        return (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess) ? prop.multiProcessorCount : 256;
    }();
    return n;
}
template <auto Kernel> int ideas_blocks_per_cu(int threads) {  // resident blocks of one kernel instantiation per CU
    static const int occ = [threads] {
        int o = 0;
        return (hipOccupancyMaxActiveBlocksPerMultiprocessor(&o, Kernel, threads, 0) == hipSuccess && o > 0) ? o : 2;
    }();
    return occ;
}

// ---- split-K sizing: `total` units (pixels or rows) of a reduction cut into `splits` shares of `per` units for each of `tiles` -----
struct SplitK { int64_t splits, per, spi = 0; };               // spi: splits per image / parts per image where a site has them
// the target: two waves of the `slots` resident blocks -- four where a share then still holds >= finer_min units (0: never)
static inline int64_t splitk_target(int64_t slots, int64_t tiles, int64_t total, int64_t finer_min) {
    int64_t s = finer_min ? (4 * slots) / tiles : 0;
    if (s < 1 || total / s < finer_min) s = (2 * slots) / tiles;
    return s < 1 ? 1 : s;
}
// shares rounded up to the pipeline step, and the number of shares that leaves
static inline SplitK splitk_round(int64_t total, int64_t splits, int64_t step) {
    const int64_t per = ideas_cdiv(ideas_cdiv(total, splits), step) * step;
    return {ideas_cdiv(total, per), per};
}
// the grid should be a whole number of waves of resident blocks: the last, partially filled wave costs as much as a full one (1026
// blocks on 1024 slots ran 2x the time).  Rounding `per` up can shave a split off; re-balance to the largest count giving whole waves.
static inline SplitK splitk_whole_waves(SplitK k, int64_t total, int64_t step, int64_t tiles, int64_t slots) {
    const int64_t blocks = tiles * k.splits, waves = blocks / slots;
    if (waves < 1 || blocks % slots == 0 || (waves * slots) / tiles < 1) return k;
    return splitk_round(total, (waves * slots) / tiles, step);
}

// <WM, WN, MT, NT> of an MFMA tile as a value: what a family's tile ladder hands to its visitor
template <int WM_, int WN_, int MT_, int NT_> struct ideas_tile {
    static constexpr int WM = WM_, WN = WN_, MT = MT_, NT = NT_, BM = WM_ * MT_ * 32, BN = WN_ * NT_ * 32;
};
// the weight-gradient tiles of the f32 and the bf16 family by output channels (o x k)
template <typename F> int ideas_wgrad_tile(const ideas_conv_params* p, F f) {
    if (p->Cout > 64) return f(ideas_tile<2, 2, 2, 2>{});  // 128 x 128
    if (p->Cout > 32) return f(ideas_tile<2, 2, 1, 2>{});  // 64 x 128
    return f(ideas_tile<1, 4, 1, 1>{});                    // 32 x 128
}

// ---- diagnostic (ideas_conv_splitk_plan, conv_igemm.hip): the plan a split-K launcher makes for *p on `slots` resident blocks
// (<= 0: the launcher's own count, returned in `slots`)
struct ideas_plan { SplitK k; int64_t slots; };
typedef ideas_plan ideas_plan_query(const ideas_conv_params* p, int scaled, int64_t slots);
ideas_plan_query ideas_wino_wgrad_plan, ideas_b3_wgrad_plan, ideas_b3_wgrad3_plan, ideas_b3_pw_wgrad_plan, ideas_bf16_wgrad_plan,
    ideas_bf16_wgrad3_plan;
