/*
 * Host-side constant setup of the FSR 1.0 hot path: FsrEasuCon, FsrEasuConOffset, FsrRcasCon.
 *
 * Bit-exact replacement of the A_CPU build of the reference (ffx-fsr/ffx_fsr1.h:156-225,
 * :662-672 with the ffx_a.h helpers AU1_AF1 :141, ARcpF1 :326, AExp2F1 :283, AU1_AH1_AF1
 * :482-549, AU1_AH2_AF2 :552).  Must be compiled without FMA contraction and without
 * fast-math (the Makefile passes -ffp-contract=off): "0.5*vp*rcp(out)-0.5" is two roundings in
 * the reference and has to stay two roundings here.
 */
#include <math.h>
#include <string.h>

#include "fsr1_hip.h"

static uint32_t bits_of(float f) {
  uint32_t u;
  memcpy(&u, &f, sizeof u);
  return u;
}

/* The reference multiplies by a reciprocal instead of dividing (ffx_fsr1.h:171-174), so
 * 2560/3840 and 1440/2160 differ in the last bit; keep that. */
static float rcp(float x) { return 1.0f / x; }

void FsrEasuCon(uint32_t* con0, uint32_t* con1, uint32_t* con2, uint32_t* con3, float inputViewportInPixelsX,
                float inputViewportInPixelsY, float inputSizeInPixelsX, float inputSizeInPixelsY,
                float outputSizeInPixelsX, float outputSizeInPixelsY) {
  const float rOutX = rcp(outputSizeInPixelsX), rOutY = rcp(outputSizeInPixelsY);
  const float rInX = rcp(inputSizeInPixelsX), rInY = rcp(inputSizeInPixelsY);
  /* con0: output pixel -> input pixel position (scale, then half-texel bias) */
  con0[0] = bits_of(inputViewportInPixelsX * rOutX);
  con0[1] = bits_of(inputViewportInPixelsY * rOutY);
  con0[2] = bits_of(0.5f * inputViewportInPixelsX * rOutX - 0.5f);
  con0[3] = bits_of(0.5f * inputViewportInPixelsY * rOutY - 0.5f);
  /* con1: texel size, and the centre of gather 0 relative to the top-left of texel 'f' */
  con1[0] = bits_of(rInX);
  con1[1] = bits_of(rInY);
  con1[2] = bits_of(1.0f * rInX);
  con1[3] = bits_of(-1.0f * rInY);
  /* con2/con3: centres of gathers 1,2,3 relative to gather 0 */
  con2[0] = bits_of(-1.0f * rInX);
  con2[1] = bits_of(2.0f * rInY);
  con2[2] = bits_of(1.0f * rInX);
  con2[3] = bits_of(2.0f * rInY);
  con3[0] = bits_of(0.0f * rInX);
  con3[1] = bits_of(4.0f * rInY);
  con3[2] = 0;
  con3[3] = 0;
}

void FsrEasuConOffset(uint32_t* con0, uint32_t* con1, uint32_t* con2, uint32_t* con3, float inputViewportInPixelsX,
                      float inputViewportInPixelsY, float inputSizeInPixelsX, float inputSizeInPixelsY,
                      float outputSizeInPixelsX, float outputSizeInPixelsY, float inputOffsetInPixelsX,
                      float inputOffsetInPixelsY) {
  FsrEasuCon(con0, con1, con2, con3, inputViewportInPixelsX, inputViewportInPixelsY, inputSizeInPixelsX,
             inputSizeInPixelsY, outputSizeInPixelsX, outputSizeInPixelsY);
  con0[2] = bits_of(0.5f * inputViewportInPixelsX * rcp(outputSizeInPixelsX) - 0.5f + inputOffsetInPixelsX);
  con0[3] = bits_of(0.5f * inputViewportInPixelsY * rcp(outputSizeInPixelsY) - 0.5f + inputOffsetInPixelsY);
}

/* float -> binary16 bit pattern by truncation of the mantissa (no rounding), denormals produced,
 * everything at or above 65520-ish, infinities and NaNs clamped to +-65504.  The reference does it
 * with two 512-entry tables indexed by sign|exponent; the tables encode exactly these four ranges. */
uint32_t AU1_AH1_AF1(float f) {
  const uint32_t u = bits_of(f);
  const uint32_t sign = (u >> 16) & 0x8000u;
  const int32_t exp = (int32_t)((u >> 23) & 0xffu) - 127; /* unbiased */
  const uint32_t man = u & 0x007fffffu;
  if (exp < -24) return sign;                       /* underflows even the smallest denormal */
  if (exp < -14) {                                  /* half denormal: hidden bit becomes explicit */
    const int sh = -14 - exp;                       /* 1..10 */
    return sign + (0x0400u >> sh) + (man >> (13 + sh));
  }
  if (exp <= 15) return sign + ((uint32_t)(exp + 15) << 10) + (man >> 13);
  return sign + 0x7bffu;
}

void FsrRcasCon(uint32_t* con, float sharpness) {
  const float linear = exp2f(-sharpness); /* stops -> linear */
  const uint32_t h = AU1_AH1_AF1(linear);
  con[0] = bits_of(linear);
  con[1] = h + (h << 16);
  con[2] = 0;
  con[3] = 0;
}

/* YCbCr -> RGB matrices for raw 8-bit codes in, RGB in {0 to 1} out (fsr1_ycbcr, include/fsr1_hip.h).  With the luma weights
 * Kr, Kb (Kg = 1 - Kr - Kb) of the standard and E'y = (Y - y0) / ys, E'pb = (Cb - 128) / cs, E'pr = (Cr - 128) / cs:
 *   R = E'y + 2 (1 - Kr) E'pr,  G = E'y - 2 Kb (1 - Kb) / Kg E'pb - 2 Kr (1 - Kr) / Kg E'pr,  B = E'y + 2 (1 - Kb) E'pb
 * (y0, ys, cs) = (16, 219, 224) for limited ("video") range, (0, 255, 255) for full range.  Every coefficient is formed in double and
 * rounded to float once. */
/* The levels of a depth: limited range is the 8-bit levels times 2^(bits - 8) (exact in double), full range 0 .. 2^bits - 1 with the
 * chroma zero at 2^(bits - 1).  0 for a depth that is not 8, 10, 12 or 16. */
typedef struct { double y0, ys, cs, c0; } levels;
static int levels_of(int full_range, int bits, levels* l) {
  if (bits != 8 && bits != 10 && bits != 12 && bits != 16) return 0;
  const double up = (double)(1u << (bits - 8)), top = (double)((1u << bits) - 1u);
  l->y0 = full_range ? 0.0 : 16.0 * up;
  l->ys = full_range ? top : 219.0 * up;
  l->cs = full_range ? top : 224.0 * up;
  l->c0 = 128.0 * up;
  return 1;
}
static int luma_weights(int standard, double* kr, double* kb) {
  static const double k[3][2] = {{0.299, 0.114}, {0.2126, 0.0722}, {0.2627, 0.0593}};  /* BT.601, BT.709, BT.2020 (non-constant luminance) */
  if (standard < FSR1_YCBCR_BT601 || standard > FSR1_YCBCR_BT2020) return 0;
  *kr = k[standard][0];
  *kb = k[standard][1];
  return 1;
}

static int ycbcr_fill(fsr1_ycbcr* y, double kr, double kb, int full_range, int bits) {
  levels l;
  if (!y || !levels_of(full_range, bits, &l)) return FSR1_ERR_INVALID_ARGUMENT;
  const double kg = 1.0 - kr - kb;
  const double y0 = l.y0, ys = l.ys, cs = l.cs;
  const double m[3][3] = {{1.0 / ys, 0.0, 2.0 * (1.0 - kr) / cs},
                          {1.0 / ys, -2.0 * kb * (1.0 - kb) / kg / cs, -2.0 * kr * (1.0 - kr) / kg / cs},
                          {1.0 / ys, 2.0 * (1.0 - kb) / cs, 0.0}};
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) y->m[r][c] = (float)m[r][c];
    y->bias[r] = (float)(-(y0 * m[r][0] + l.c0 * (m[r][1] + m[r][2])));
  }
  y->siting = FSR1_CHROMA_LEFT;
  y->chroma_offset_bytes = 0;
  return FSR1_OK;
}

int fsr1_ycbcr_bt601(fsr1_ycbcr* ycbcr, int full_range) { return ycbcr_fill(ycbcr, 0.299, 0.114, full_range, 8); }
int fsr1_ycbcr_bt709(fsr1_ycbcr* ycbcr, int full_range) { return ycbcr_fill(ycbcr, 0.2126, 0.0722, full_range, 8); }
int fsr1_ycbcr_fill(fsr1_ycbcr* ycbcr, int standard, int full_range, int bits) {
  double kr, kb;
  if (!luma_weights(standard, &kr, &kb)) return FSR1_ERR_INVALID_ARGUMENT;
  return ycbcr_fill(ycbcr, kr, kb, full_range, bits);
}

/* RGB -> YCbCr matrices for RGB in {0 to 1} in, codes 0 .. 255 out (fsr1_rgb2ycbcr, include/fsr1_hip.h), from the same Kr, Kb:
 *   Y = y0 + ys (Kr R + Kg G + Kb B),  Cb = 128 + cs (B - E'y) / (2 (1 - Kb)),  Cr = 128 + cs (R - E'y) / (2 (1 - Kr))
 * with E'y = Kr R + Kg G + Kb B.  Every coefficient is formed in double and rounded to float once. */
static int rgb2ycbcr_fill(fsr1_rgb2ycbcr* y, double kr, double kb, int full_range, int bits) {
  levels l;
  if (!y || !levels_of(full_range, bits, &l)) return FSR1_ERR_INVALID_ARGUMENT;
  const double kg = 1.0 - kr - kb;
  const double y0 = l.y0, ys = l.ys, cs = l.cs;
  const double cb = cs / (2.0 * (1.0 - kb)), cr = cs / (2.0 * (1.0 - kr));
  const double m[3][3] = {{ys * kr, ys * kg, ys * kb}, {-cb * kr, -cb * kg, cb * (1.0 - kb)}, {cr * (1.0 - kr), -cr * kg, -cr * kb}};
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) y->m[r][c] = (float)m[r][c];
    y->bias[r] = (float)(r ? l.c0 : y0);
  }
  y->siting = FSR1_CHROMA_CENTER;
  y->chroma_offset_bytes = 0;
  return FSR1_OK;
}

int fsr1_rgb2ycbcr_bt601(fsr1_rgb2ycbcr* ycbcr, int full_range) { return rgb2ycbcr_fill(ycbcr, 0.299, 0.114, full_range, 8); }
int fsr1_rgb2ycbcr_bt709(fsr1_rgb2ycbcr* ycbcr, int full_range) { return rgb2ycbcr_fill(ycbcr, 0.2126, 0.0722, full_range, 8); }
int fsr1_rgb2ycbcr_fill(fsr1_rgb2ycbcr* ycbcr, int standard, int full_range, int bits) {
  double kr, kb;
  if (!luma_weights(standard, &kr, &kb)) return FSR1_ERR_INVALID_ARGUMENT;
  return rgb2ycbcr_fill(ycbcr, kr, kb, full_range, bits);
}
