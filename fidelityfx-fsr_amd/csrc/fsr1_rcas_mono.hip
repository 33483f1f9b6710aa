// RCAS on single-channel images (FSR1_FORMAT_R16F / R32F / R8_UNORM): the strip kernel of fsr1_rcas_planar.hip for one plane — no LDS,
// no barrier.  The strip itself, and what it does, is in fsr1_rcas_mono_kernel.h (shared with fsr1_rcas_luma.hip).
#include "fsr1_rcas_mono_kernel.h"

namespace fsr1 {

// OPTS = false: the plain pass (no denoise / HDR square), flags compiled out.  RING: raw rows in flight per lane.  G: columns per lane.
template <int FMT, bool EXACT, bool OPTS, bool WIDE, int RING, int G>
__global__ void __launch_bounds__(kRcasMonoThreads) rcas_mono_kernel(const RcasArgs a) {
  rcas_mono_tile<FMT, EXACT, OPTS, WIDE, RING, G>(a, xcd_swizzle(blockIdx.x, a.tiles_x * a.tiles_y * a.frames, a.xcd_shift));
}

static int rcas_mono_cols(int fmt) { return fmt == FSR1_FORMAT_R32F ? 2 : 4; }

// Strip height by fsr1_rcas.hip's rule on this kernel's waves: 16 rows unless that leaves fewer than four waves per SIMD (and the launch
// does not run beside other frames' launches), then 8 — a 4K frame: 4050 waves of 8 rows.  (4-row strips read half as many rows again as
// they store and measured no faster: fsr1_rcas_mono_kernel.h.)
void rcas_mono_geometry(int fmt, int width, int height, int frames, bool overlapped, int cus, int* tiles_x, int* tiles_y, int* rows) {
  const int wave_cols = 64 * rcas_mono_cols(fmt);
  int r = 16;
  if (!overlapped && (long long)((width + wave_cols - 1) / wave_cols) * ((height + r - 1) / r) * frames < 4LL * 4 * cus) r = 8;
  *rows = r;
  *tiles_x = (width + wave_cols * kRcasMonoWaves - 1) / (wave_cols * kRcasMonoWaves);
  *tiles_y = (height + r - 1) / r;
}

// bytes a lane's group moves as one access (what `wide` has to be checked against)
size_t rcas_mono_access_bytes(int fmt) { return fmt == FSR1_FORMAT_R8_UNORM ? 4 : 8; }

template <int FMT, bool EXACT, bool OPTS>
static void rcas_mono_launch_one(const RcasArgs& a, bool wide, hipStream_t stream) {
  const dim3 grid((unsigned)(a.tiles_x * a.tiles_y * a.frames)), block(kRcasMonoThreads);
  if (wide) hipLaunchKernelGGL((rcas_mono_kernel<FMT, EXACT, OPTS, true, kRcasMonoRing, kRcasMonoCols<FMT>>), grid, block, 0, stream, a);
  else hipLaunchKernelGGL((rcas_mono_kernel<FMT, EXACT, OPTS, false, kRcasMonoRing, kRcasMonoCols<FMT>>), grid, block, 0, stream, a);
}

// wide: the lanes' groups move as one access (the host has checked both images' base, pitch and frame stride against it).
hipError_t rcas_mono_launch(const RcasArgs& a, int fmt, bool exact, bool wide, hipStream_t stream) {
  const bool opts = (a.flags & (FSR1_FLAG_RCAS_DENOISE | FSR1_FLAG_HDR_SQUARE)) != 0;
#define FSR1_RCASM_O(F, E) do { if (opts) rcas_mono_launch_one<F, E, true>(a, wide, stream); else rcas_mono_launch_one<F, E, false>(a, wide, stream); } while (0)
#define FSR1_RCASM_E(F) do { if (exact) FSR1_RCASM_O(F, true); else FSR1_RCASM_O(F, false); } while (0)
  switch (fmt) {
    case FSR1_FORMAT_R16F: FSR1_RCASM_E(FSR1_FORMAT_R16F); break;
    case FSR1_FORMAT_R32F: FSR1_RCASM_E(FSR1_FORMAT_R32F); break;
    case FSR1_FORMAT_R8_UNORM: FSR1_RCASM_E(FSR1_FORMAT_R8_UNORM); break;
    default: return hipErrorInvalidValue;
  }
#undef FSR1_RCASM_E
#undef FSR1_RCASM_O
  return hipGetLastError();
}

}  // namespace fsr1
