// NV12 output (FSR1_FORMAT_NV12 as the image a pass stores): the RGB -> YCbCr conversion and the code store pinned in fsr1_hip.h
// ("THE PINNED CONVERSION, RGB -> NV12"), for a kernel that holds the binary32 RGB results of a 2 x 2 block's pixels in registers.
// The luma of a pixel is a function of that pixel; the chroma pair of a block is a function of the block's average (or of its top-left
// pixel), formed per channel of R, G, B first — so a kernel needs the horizontal sums of two rows and nothing else.
#pragma once
#include "fsr1_device_rcas.hpp"

namespace fsr1 {

// device side of fsr1_rgb2ycbcr
struct Rgb2YcbcrView {
  float m[3][3];  // rows Y, Cb, Cr; columns R, G, B
  float bias[3];
  int siting;               // FSR1_CHROMA_CENTER or FSR1_CHROMA_REPLICATE (the host has refused everything else)
  long long chroma_offset;  // bytes from a frame's first Y byte to its first Cb byte
  float max_code;           // 2^bits - 1: 255 (NV12), 1023 (P010), 65535 (P016)
  uint32_t shift;           // 16 - bits of a 16-bit format: a stored word is code << shift (P010: the six low bits are zero); NV12: 0
};

// Row k of the matrix on one RGB value: bias + m0 R, + m1 G, + m2 B with every product and every sum rounded to binary32 by itself.
__device__ __forceinline__ float nv12_component(const Rgb2YcbcrView& c, int k, rgb_t p) {
#pragma clang fp contract(off)
  float t = __fadd_rn(c.bias[k], __fmul_rn(c.m[k][0], p.r));
  t = __fadd_rn(t, __fmul_rn(c.m[k][1], p.g));
  return __fadd_rn(t, __fmul_rn(c.m[k][2], p.b));
}

// The code of a component: the project's UNORM store rule in code units — clamp, one rounded addition of a half, truncation.
// fmaxf is IEEE maxNum: a NaN becomes 0.  max_code, shift: of the format's depth — the result is the word (or byte) the surface holds,
// code << shift; 65535.5 is a binary32 number, so the rounded addition is what it says at 16 bits too.
__device__ __forceinline__ uint32_t nv12_code(float v, float max_code = 255.0f, uint32_t shift = 0) {
#pragma clang fp contract(off)
  return (uint32_t)__fadd_rn(fminf(fmaxf(v, 0.0f), max_code), 0.5f) << shift;
}

__device__ __forceinline__ uint32_t nv12_luma_code(const Rgb2YcbcrView& c, rgb_t p) { return nv12_code(nv12_component(c, 0, p)); }
// 16-bit words (P010 / P016): the Y word, and the (Cb, Cr) pair as the aligned dword the surface holds, Cb in the low word
__device__ __forceinline__ uint32_t p016_luma_word(const Rgb2YcbcrView& c, rgb_t p) { return nv12_code(nv12_component(c, 0, p), c.max_code, c.shift); }
__device__ __forceinline__ uint32_t p016_pair_words(const Rgb2YcbcrView& c, rgb_t a) {
  return nv12_code(nv12_component(c, 1, a), c.max_code, c.shift) | (nv12_code(nv12_component(c, 2, a), c.max_code, c.shift) << 16);
}

// The (Cb, Cr) pair of a block from its chroma sample `a`, as the 16 bits the surface holds: Cb in the low byte.
__device__ __forceinline__ uint32_t nv12_pair_code(const Rgb2YcbcrView& c, rgb_t a) {
  return nv12_code(nv12_component(c, 1, a)) | (nv12_code(nv12_component(c, 2, a)) << 8);
}

// Per channel the sum of two horizontally adjacent pixels (s0 or s1 of the box), and the box sample 0.25 (s0 + s1): the scaling is exact.
__device__ __forceinline__ rgb_t nv12_sum(rgb_t p, rgb_t q) { return rgb_t{p.r + q.r, p.g + q.g, p.b + q.b}; }
__device__ __forceinline__ rgb_t nv12_box(rgb_t s0, rgb_t s1) { return rgb_t{0.25f * (s0.r + s1.r), 0.25f * (s0.g + s1.g), 0.25f * (s0.b + s1.b)}; }

}  // namespace fsr1
