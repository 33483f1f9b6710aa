// Colour stages in packed binary16 (parity class "H"): FsrSrtmHx2 / FsrLfgaHx2 / FsrSrtmInvHx2 / FsrTepdC8Hx2 | C10Hx2 with
// FsrTepdDitHx2's per-lane formula (ffx-fsr/ffx_fsr1.h:1017-1024, :1048-1056, :1124-1198) on a PAIR of pixels held in the two
// halves of packed registers.  Each reference operation is one native binary16 operation (contraction off), so the result is
// bit-identical to the CPU-evaluated H path.  Shared by the stand-alone colour pass (fsr1_color.hip) and by the prologue /
// epilogue variants of the EASU-H and RCAS-H kernels: the prologue is SRTM on a texel as it is loaded, the epilogue is
// LFGA -> SRTM_INV -> TEPD on the result for an output pixel — the F stages' split (fsr1_device_color.hpp), noise slice and
// offsets included (ColorArgs as the host prepares it).
//
// Included from fsr1_device_half.hpp (which defines rgbh2_t); including this header first works as well.
#pragma once
#include "fsr1_device_half.hpp"
#include "fsr1_device_color.hpp"

namespace fsr1 {

__device__ __forceinline__ half2_t c_h2(half_t a, half_t b) { return half2_t{a, b}; }
__device__ __forceinline__ half2_t c_h2s(half_t a) { return half2_t{a, a}; }
__device__ __forceinline__ half2_t c_max2(half2_t a, half2_t b) { return __builtin_elementwise_max(a, b); }
__device__ __forceinline__ half2_t c_min2(half2_t a, half2_t b) { return __builtin_elementwise_min(a, b); }
__device__ __forceinline__ half2_t c_sat2(half2_t a) { return c_min2(c_max2(a, c_h2s((half_t)0.0f)), c_h2s((half_t)1.0f)); }
__device__ __forceinline__ half2_t c_rcp2(half2_t a) { return half2_t{half_rcp(a.x), half_rcp(a.y)}; }  // ARcpH2: correctly rounded 1/x
// correctly rounded binary16 sqrt: the binary32 sqrt (correctly rounded) narrowed RTNE is exact-rounding because 24 >= 2*11+2
__device__ __forceinline__ half2_t c_sqrt2(half2_t a) { return half2_t{(half_t)sqrtf((float)a.x), (half_t)sqrtf((float)a.y)}; }
__device__ __forceinline__ half2_t c_floor2(half2_t a) { return half2_t{(half_t)__builtin_floorf16(a.x), (half_t)__builtin_floorf16(a.y)}; }
// ffx_a.h:1815 APrxMedRcpH2
__device__ __forceinline__ half2_t APrxMedRcpH2(half2_t a) {
  typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
  const u16x2 ai = __builtin_bit_cast(u16x2, a);
  const u16x2 bi = {(unsigned short)(0x778du - ai.x), (unsigned short)(0x778du - ai.y)};
  const half2_t b = __builtin_bit_cast(half2_t, bi);
  return b * (-b * a + c_h2s((half_t)2.0f));
}
__device__ __forceinline__ half2_t AGtZeroH2(half2_t m) { return c_sat2(m * c_h2s((half_t)__builtin_inff())); }  // ffx_a.h:1525
__device__ __forceinline__ half2_t FsrTepdCHx2(half2_t c, half2_t dit, half_t k, half_t rk) {  // :1153-1198, one channel
  half2_t n = c_sqrt2(c);
  n = c_floor2(n * c_h2s(k)) * c_h2s(rk);
  const half2_t a = n * n;
  half2_t b = n + c_h2s(rk);
  b = b * b;
  const half2_t r = (c - b) * APrxMedRcpH2(a - b);
  return c_sat2(n + AGtZeroH2(dit - r) * c_h2s(rk));
}

// Prologue: FsrSrtmHx2 (:1052-1053) on a pair of texels as they are loaded.  FsrSrtmH(0) == 0, so a tap outside the image stays 0.
__device__ __forceinline__ void color_prologue_h2(const ColorArgs& ca, rgbh2_t& c) {
  if (ca.stages & FSR1_COLOR_SRTM) {
    const half2_t rcp = c_rcp2(c_max2(c.r, c_max2(c.g, c.b)) + c_h2s((half_t)1.0f));
    c.r = c.r * rcp; c.g = c.g * rcp; c.b = c.b * rcp;
  }
}

// Epilogue on the results for output pixels (x0, y) and (x1, y) (.x / .y of every register): LFGA -> SRTM_INV -> TEPD.
// x0 and x1 are separate: a kernel's pair need not be adjacent (and a lane with one pixel passes it twice).
__device__ __forceinline__ void color_epilogue_h2(const ColorArgs& ca, uint32_t x0, uint32_t x1, uint32_t y, rgbh2_t& c) {
  const uint32_t st = ca.stages;
  const half_t one = (half_t)1.0f;
  float4_t n0 = {0.f, 0.f, 0.f, 0.f}, n1 = n0;
  if (st & kColorNeedsNoise) { n0 = noise_fetch(ca.noise, x0, y); n1 = noise_fetch(ca.noise, x1, y); }
  if (st & FSR1_COLOR_LFGA) {  // :1022-1023
    const half2_t amount = c_h2s((half_t)ca.amount), bias = c_h2s((half_t)ca.bias);
    const half2_t tR = c_h2((half_t)n0.x, (half_t)n1.x) + bias, tG = c_h2((half_t)n0.y, (half_t)n1.y) + bias, tB = c_h2((half_t)n0.z, (half_t)n1.z) + bias;
    c.r = c.r + (tR * amount) * c_min2(c_h2s(one) - c.r, c.r);
    c.g = c.g + (tG * amount) * c_min2(c_h2s(one) - c.g, c.g);
    c.b = c.b + (tB * amount) * c_min2(c_h2s(one) - c.b, c.b);
  }
  if (st & FSR1_COLOR_SRTM_INV) {  // :1054-1055
    const half2_t rcp = c_rcp2(c_max2(c_h2s((half_t)(1.0 / 32768.0)), c_h2s(one) - c_max2(c.r, c_max2(c.g, c.b))));
    c.r = c.r * rcp; c.g = c.g * rcp; c.b = c.b * rcp;
  }
  if (st & (FSR1_COLOR_TEPD_C8 | FSR1_COLOR_TEPD_C10)) {
    const bool c8 = (st & FSR1_COLOR_TEPD_C8) != 0;
    const half_t k = c8 ? (half_t)255.0f : (half_t)1023.0f, rk = c8 ? (half_t)(1.0 / 255.0) : (half_t)(1.0 / 1023.0);
    // :1153-1160 FsrTepdDitHx2 is FsrTepdDitH per lane: binary32 arithmetic, narrowed once
    const half2_t dit = (st & FSR1_COLOR_DITHER_FROM_NOISE) ? c_sat2(c_h2((half_t)n0.w, (half_t)n1.w))
                                                            : c_h2((half_t)FsrTepdDitF(x0, y, ca.frame), (half_t)FsrTepdDitF(x1, y, ca.frame));
    c.r = FsrTepdCHx2(c.r, dit, k, rk); c.g = FsrTepdCHx2(c.g, dit, k, rk); c.b = FsrTepdCHx2(c.b, dit, k, rk);
  }
}

}  // namespace fsr1
