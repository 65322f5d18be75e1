// Wave64 helpers the gfx950 kernels share: 32-bit DPP reductions, an inclusive scan, the intra-wave fence, one s_waitcnt.
#pragma once
#include <hip/hip_runtime.h>

namespace aegis {

// One level of a DPP reduction: the lane's value combined with that of the lane CTRL names.  A lane CTRL gives no source
// (and the rows ROW_MASK leaves out) reads the identity instead for the unsigned max / min -- the level is then one
// v_max_u32_dpp / v_min_u32_dpp -- and its own value for the signed min and the or.
enum DppOp { dpp_umax, dpp_umin, dpp_imin, dpp_or };
template <DppOp OP, int CTRL, int ROW_MASK>
__device__ __forceinline__ int dpp_level(int v) {
    const int o = __builtin_amdgcn_update_dpp(OP == dpp_umax ? 0 : OP == dpp_umin ? -1 : v, v, CTRL, ROW_MASK, 0xf, false);
    if (OP == dpp_umax) return (int)max((unsigned)v, (unsigned)o);
    if (OP == dpp_umin) return (int)min((unsigned)v, (unsigned)o);
    return OP == dpp_imin ? min(v, o) : (v | o);
}
// The ladder: uniform result, or (ROWS) after the four shifts lane 15 of each row of 16 lanes holds its row's result.
template <DppOp OP, bool ROWS = false>
__device__ __forceinline__ int wave_reduce(int v) {
    v = dpp_level<OP, 0x111, 0xf>(v);   // row_shr:1
    v = dpp_level<OP, 0x112, 0xf>(v);   // row_shr:2
    v = dpp_level<OP, 0x114, 0xf>(v);   // row_shr:4
    v = dpp_level<OP, 0x118, 0xf>(v);   // row_shr:8
    if (ROWS) return v;
    v = dpp_level<OP, 0x142, 0xa>(v);   // row_bcast:15
    v = dpp_level<OP, 0x143, 0xc>(v);   // row_bcast:31
    return __builtin_amdgcn_readlane(v, 63);
}
__device__ __forceinline__ unsigned wave_umax(unsigned v) { return (unsigned)wave_reduce<dpp_umax>((int)v); }
__device__ __forceinline__ unsigned wave_umin(unsigned v) { return (unsigned)wave_reduce<dpp_umin>((int)v); }
__device__ __forceinline__ unsigned row16_umin(unsigned v) { return (unsigned)wave_reduce<dpp_umin, true>((int)v); }
__device__ __forceinline__ int wave_min_i32(int v) { return wave_reduce<dpp_imin>(v); }
__device__ __forceinline__ unsigned wave_or_u32(unsigned v) { return (unsigned)wave_reduce<dpp_or>((int)v); }

__device__ __forceinline__ int wave_incl_scan(int v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int nb = __shfl_up(v, o);
        if (lane >= o) v += nb;
    }
    return v;
}

// A double moved one lane up the wave: lane l receives lane l - 1's v, lane 0 keeps `first`.  The two halves go through one
// DPP move each (wave_shr:1, which gfx9 still has: the shift crosses the rows of 16 lanes).
__device__ __forceinline__ double wave_shr1_f64(double v, double first) {
    const long long b = __double_as_longlong(v), f = __double_as_longlong(first);
    const int lo = __builtin_amdgcn_update_dpp((int)f, (int)b, 0x138, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp((int)(f >> 32), (int)(b >> 32), 0x138, 0xf, 0xf, false);
    return __longlong_as_double(((long long)hi << 32) | (unsigned)lo);
}
// lane `src`'s double in every lane; src is the same in all of them
__device__ __forceinline__ double wave_readlane_f64(double v, int src) {
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_readlane((int)b, src), hi = __builtin_amdgcn_readlane((int)(b >> 32), src);
    return __longlong_as_double(((long long)hi << 32) | (unsigned)lo);
}

// orders a wave's own LDS traffic where its lanes hand data to each other; the other waves are not involved
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// s_waitcnt immediate, gfx9 encoding ONLY (vmcnt in bits 3:0 and 15:14, expcnt 6:4, lgkmcnt 11:8): vmcnt(0), expcnt and
// lgkmcnt left alone.  gfx10 and later encode the counters differently (and count stores in a counter of their own).
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__GFX9__)
#error "kWaitVmcnt0 is a gfx9 s_waitcnt encoding: this code is built for gfx950"
#endif
constexpr int kWaitVmcnt0 = 0x0F70;

}  // namespace aegis
