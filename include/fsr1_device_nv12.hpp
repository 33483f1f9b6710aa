// NV12 input (FSR1_FORMAT_NV12: a full-resolution 8-bit Y plane and a half-resolution plane of interleaved Cb, Cr pairs — what a
// hardware decoder writes) for the tiled EASU form: phase 1 of the footprint staging with the chroma reconstruction and the
// YCbCr -> RGB conversion pinned in fsr1_hip.h folded in.  The conversion costs a dozen operations per INPUT texel and phase 1
// touches every footprint texel exactly once, so it needs no pass and no image of its own.  What the staging leaves in LDS are
// the records of every other EASU kernel (R, G, B, luma*2 | analysis): phases 2 and 3 and the plane stores are
// fsr1_device_planar.hpp's, unchanged.
//
// Phase 1 has two steps.  (1) The tile's CHROMA footprint — the pairs any of its luma texels can ask for, at most
// (fw / 2 + 3) x (fh / 2 + 3) of them, 20 x 8 = 320 bytes at exactly 2x — goes into an LDS region of its own as raw 16-bit pairs:
// one wave per chroma row with a scalar row base, one lane per pair, the plane's clamp applied while loading, so that slot (r, s)
// holds pair (clamp(cj0 + r), clamp(ck0 + s)) and a reader never clamps again.  (2) One lane per luma footprint column, one wave
// per footprint row as in easu_stage_footprint_planar: a lane loads ONE Y byte per texel, reads its four chroma pairs from LDS,
// reconstructs, converts and writes one 16-byte record.  A wave issues the Y loads of its first trip BEFORE it stages the chroma
// pairs, so both sets of global loads are in flight together and the barrier between the steps waits for memory once.
// Every global access is one or two bytes wide: base, pitch, chroma offset and frame stride need only be multiples of two.
//
// P010 / P016 (FSR1_FORMAT_P010 / P016: the same arrangement in 16-bit words, the code in the upper `bits` bits) take the same two steps
// with the word width as a compile-time parameter (WORD = uint16_t) and the depth as a run-time, wave-uniform shift (Nv12View::shift),
// as the siting is: a lane loads one Y WORD per texel, the chroma region holds 32-bit pairs (640 bytes at exactly 2x), and every global
// access is one word or one aligned dword.  The read side is its own.  A texel's pair and the pair its reconstruction blends with are
// ADJACENT dword slots, so the lane reads the LOWER of the two and its right neighbour — one ds_read2_b32 per chroma row, two per texel
// where the 8-bit form issues four ds_read_u16 — and folds "which of the two is mine" into the blend weight instead of selecting:
// own + w (other - own) = left + w' (right - left) with w' = w for an odd texel (own = left) and 1 - w for an even one (own = right).
// Both sides are exact in binary32 (below), so they are the same number and the form costs no v_cndmask at all.
#pragma once
#include "fsr1_device_planar.hpp"

namespace fsr1 {

// device side of fsr1_ycbcr
struct Nv12View {
  float m[3][3];
  float bias[3];
  int siting;               // FSR1_CHROMA_*
  long long chroma_offset;  // bytes from a frame's first Y byte to its first Cb byte
  int shift;                // WORD = uint16_t: 16 - bits, the code of a word is word >> shift (P010: 6, P016: 0); unused by NV12
};

// what the chroma region of LDS holds per (Cb, Cr) pair
template <class WORD> struct Nv12Pair;
template <> struct Nv12Pair<uint8_t> { typedef uint16_t T; };
template <> struct Nv12Pair<uint16_t> { typedef uint32_t T; };

// chroma pairs a footprint of f luma texels can ask for along one axis: texels xa .. xa + f - 1 lie in pairs xa / 2 .. xa / 2 + f / 2,
// and every reconstruction reads at most one pair either side
__host__ __device__ constexpr int nv12_chroma_extent(int f) { return (f >> 1) + 3; }
__host__ __device__ constexpr size_t nv12_chroma_lds_bytes(int fw, int fh, int pair_bytes = 2) {
  return ((size_t)nv12_chroma_extent(fw) * (size_t)nv12_chroma_extent(fh) * (size_t)pair_bytes + 15) & ~(size_t)15;
}

// The pinned conversion (fsr1_hip.h): per channel bias + m0 Y, + m1 Cb, + m2 Cr with every product and every sum rounded to binary32
// by itself, then the clamp to {0 to 1}; luma*2 is the reference's expression on the result, as in every other staging function.
__device__ __forceinline__ float4_t nv12_record(const Nv12View& c, float y, float cb, float cr) {
#pragma clang fp contract(off)
  float v[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    float t = __fadd_rn(c.bias[k], __fmul_rn(c.m[k][0], y));
    t = __fadd_rn(t, __fmul_rn(c.m[k][1], cb));
    t = __fadd_rn(t, __fmul_rn(c.m[k][2], cr));
    v[k] = fminf(fmaxf(t, 0.0f), 1.0f);
  }
  return float4_t{v[0], v[1], v[2], fmaf(v[2], 0.5f, fmaf(v[0], 0.5f, v[1]))};  // :363-366, as easu_stage_footprint
}

// Phases 1 and 2 for the footprint [fx0, fx0 + fw) x [fy0, fy0 + fh) of LUMA texels of an NV12 frame (unclamped coordinates; EASU's
// clamp-to-edge acts on them first, the chroma indices that follow are clamped to the chroma plane).  `pairs`: the LDS region of
// nv12_chroma_lds_bytes(capacity, sizeof *pairs) behind the EASU records.  WORD: uint8_t (NV12) or uint16_t (P010 / P016).  FW, FH: compile-time footprint extent (the exact-2x tiles), 0 = run-time.
// Footprints wider than a wave (minification) walk their columns — and their chroma pairs — in chunks of 64 in the same form.
// All THREADS threads of the workgroup must make the call.
template <bool EXACT, int FW = 0, int FH = 0, int THREADS = 256, class WORD = uint8_t>
__device__ __forceinline__ void easu_stage_footprint_nv12(const EasuLds& l, typename Nv12Pair<WORD>::T* pairs, const ImageView& in, const Nv12View& yc,
                                                          const char* in_frame, int fx0, int fy0, int fw_rt, int fh_rt, int tid) {
  static_assert(FW <= 64 && THREADS % 64 == 0, "one lane per footprint column");
  typedef typename Nv12Pair<WORD>::T pair_t;
  constexpr bool kWords = sizeof(WORD) == 2;
  constexpr int kWaves = THREADS / 64;
  constexpr int kU = FH ? (FH + kWaves - 1) / kWaves : 5;                       // luma rows per wave and trip
  constexpr int kCU = FH ? (nv12_chroma_extent(FH) + kWaves - 1) / kWaves : 4;  // chroma rows per wave and trip
  const int fw = FW ? FW : fw_rt, fh = FH ? FH : fh_rt;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int W = in.width, H = in.height, cw = (W + 1) >> 1, ch = (H + 1) >> 1;
  // the chroma window, from the CLAMPED footprint (whatever the constants point at, every texel the lanes read lies in
  // [xa, xa + fw) x [ya, ya + fh) of the image): slot (r, s) = pair (cj0 + r, ck0 + s), one spare slot either side
  const int ck0 = (min(max(fx0, 0), W - 1) >> 1) - 1, cj0 = (min(max(fy0, 0), H - 1) >> 1) - 1;
  const int cfw = nv12_chroma_extent(fw), cfh = nv12_chroma_extent(fh);
  const int sit = yc.siting;
  // weight of the vertical neighbour (rows are centred between two chroma rows unless the pair is replicated): wave-uniform
  const float wv = sit == FSR1_CHROMA_REPLICATE ? 0.0f : 0.25f;

  // a lane's column of the chunk that starts at footprint column c0
  struct Column {
    bool active;    // inside the footprint
    uint32_t xoff;  // byte offset of the (clamped) texel in a Y row
    int slot, d;    // chroma slot of the texel's own pair, and the step (+-1) to the pair its reconstruction blends with
    float wh;       // weight of that neighbour
    // (16-bit words: slot = the LOWER of the two slots, wh = the weight of the slot to its right, d unused)
  };
  auto column = [&](int c0) {
    const int x = min(max(fx0 + c0 + lane, 0), W - 1), odd = x & 1;
    Column c;
    c.active = c0 + lane < fw;
    c.xoff = (uint32_t)x * (uint32_t)sizeof(WORD);
    c.slot = (x >> 1) - ck0;
    c.d = odd ? 1 : -1;
    // CENTER: a quarter of the pair on the texel's own side; LEFT: even texels sit on their pair, odd ones half way to the next
    c.wh = sit == FSR1_CHROMA_CENTER ? 0.25f : (sit == FSR1_CHROMA_LEFT && odd ? 0.5f : 0.0f);
    if constexpr (kWords) {  // an even texel's neighbour is the slot on its left (the window keeps one spare slot either side)
      c.slot -= odd ? 0 : 1;
      c.wh = odd ? c.wh : 1.0f - c.wh;  // 1, 0.75 or 0.5: exact
    }
    return c;
  };
  auto load_rows = [&](const Column& c, int ly0, WORD (&yv)[kU]) {
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      const int ly = ly0 + kWaves * u;  // wave-uniform
      if (ly < fh && c.active) yv[u] = *reinterpret_cast<const WORD*>(in_frame + (long long)min(max(fy0 + ly, 0), H - 1) * in.pitch + (size_t)c.xoff);
    }
  };
  // Reconstruction: horizontally, then vertically, as a + w (b - a).  The operands are 8-bit codes and the weights quarters and
  // halves, so every difference, product and sum is exact in binary32 and equals the weighted form fsr1_hip.h writes down.
  // 16-bit words: a code has at most 16 significant bits, a horizontal blend (weights in quarters) 18, the vertical one on top of it
  // (a quarter again) 20 — of binary32's 24: still exact, in any operation order, the left + w' (right - left) form included.
  auto convert_rows = [&](const Column& c, int c0, int ly0, const WORD (&yv)[kU]) {
    if (!c.active) return;
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      const int ly = ly0 + kWaves * u;
      if (ly < fh) {
        const int gy = min(max(fy0 + ly, 0), H - 1);  // wave-uniform, like the two slot rows
        const pair_t* const p0 = pairs + ((gy >> 1) - cj0) * cfw + c.slot;
        const pair_t* const p1 = p0 + ((gy & 1) ? cfw : -cfw);
        if constexpr (kWords) {
          // two adjacent dwords per chroma row: one ds_read2_b32 each.  The code of a word: the upper 16 - shift bits (a bit-field
          // extract for Cb, a shift for Cr), so P010's six low bits never reach the arithmetic.
          const uint32_t l0 = p0[0], r0 = p0[1], l1 = p1[0], r1 = p1[1];
          const uint32_t sh = (uint32_t)yc.shift;
          auto blend = [&](bool cr) {
            auto code = [&](uint32_t v) { return (float)(cr ? v >> (16u + sh) : __builtin_amdgcn_ubfe(v, sh, 16u - sh)); };
            const float fl0 = code(l0), fr0 = code(r0), fl1 = code(l1), fr1 = code(r1);
            const float h0 = fmaf(c.wh, fr0 - fl0, fl0), h1 = fmaf(c.wh, fr1 - fl1, fl1);
            return fmaf(wv, h1 - h0, h0);
          };
          l.tex[ly * fw + c0 + lane] = nv12_record(yc, (float)((uint32_t)yv[u] >> sh), blend(false), blend(true));
        } else {
          const uint32_t a0 = p0[0], b0 = p0[c.d], a1 = p1[0], b1 = p1[c.d];
          auto blend = [&](int shift) {
            const float fa0 = (float)((a0 >> shift) & 0xffu), fb0 = (float)((b0 >> shift) & 0xffu);
            const float fa1 = (float)((a1 >> shift) & 0xffu), fb1 = (float)((b1 >> shift) & 0xffu);
            const float h0 = fmaf(c.wh, fb0 - fa0, fa0), h1 = fmaf(c.wh, fb1 - fa1, fa1);
            return fmaf(wv, h1 - h0, h0);
          };
          l.tex[ly * fw + c0 + lane] = nv12_record(yc, (float)yv[u], blend(0), blend(8));
        }
      }
    }
  };

  // ---- phase 1: the Y loads of the first trip, the chroma pairs -> LDS, a barrier, then the records ----
  WORD yv[kU];
  const Column first = column(0);
  load_rows(first, wave, yv);
  const char* const chroma = in_frame + yc.chroma_offset;
  for (int s0 = 0; s0 < cfw; s0 += 64) {  // (one trip unless the footprint is wider than 122 texels)
    const int s = s0 + lane;
    const uint32_t coff = (uint32_t)min(max(ck0 + s, 0), cw - 1) * (uint32_t)sizeof(pair_t);
    if (s < cfw) {
#pragma unroll 1
      for (int r0 = wave; r0 < cfh; r0 += kWaves * kCU) {
        pair_t cv[kCU];
#pragma unroll
        for (int u = 0; u < kCU; ++u) {
          const int r = r0 + kWaves * u;  // wave-uniform
          if (r < cfh) cv[u] = *reinterpret_cast<const pair_t*>(chroma + (long long)min(max(cj0 + r, 0), ch - 1) * in.pitch + (size_t)coff);
        }
#pragma unroll
        for (int u = 0; u < kCU; ++u) {
          const int r = r0 + kWaves * u;
          if (r < cfh) pairs[r * cfw + s] = cv[u];
        }
      }
    }
  }
  __syncthreads();
  convert_rows(first, 0, wave, yv);
  // what one trip does not cover: more than kU rows per wave, columns beyond the first 64 (run-time footprints only)
  if constexpr (!(FW && FH)) {
#pragma unroll 1
    for (int c0 = 0; c0 < fw; c0 += 64) {
      const Column c = column(c0);
#pragma unroll 1
      for (int ly0 = c0 ? wave : wave + kWaves * kU; ly0 < fh; ly0 += kWaves * kU) {
        load_rows(c, ly0, yv);
        convert_rows(c, c0, ly0, yv);
      }
    }
  }
  easu_stage_analysis<EXACT, FW, THREADS>(l, fw, fh, tid);
}

}  // namespace fsr1
