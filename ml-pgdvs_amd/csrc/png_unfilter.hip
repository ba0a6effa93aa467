// The row filters of a batch of inflated PNG images, undone on the device (the second launch of pgdvs_png_decode,
// csrc/png_inflate.hip; the filters themselves: unfilter_byte in csrc/png_inflate_core.h).
//
// Pixel (x, y) needs only its left, upper and upper-left neighbours, so one wavefront takes 64 consecutive rows on a skew:
// lane r is on row base + r and one pixel behind lane r - 1 -- at step k on pixel k - r.  A pixel is a packed word of up to
// four bytes.  What lane r - 1 finished in the step before is the pixel above (wave_prev_lane of wave.h), what it was handed there is
// the upper-left one, what lane r finished itself is the left one; each lane applies its own row's filter.  Lane 0 reads
// the row above from the stream's carry row in the workspace, where lane 63 of the row block in front stored its
// reconstructed row (63 pixels behind lane 0's reads of the same row block, which run at most kGroup - 1 pixels ahead of
// its step: a pixel is read before it is replaced; the inflated rows themselves stay as they are).  Row blocks of one image
// follow each other, images of a batch run side by side (the grid).  The same pass
// drops the filter byte and, for out_channels < channels, the alpha byte, and writes [H,W,out_channels] with the caller's
// row stride.  A stream of samples below a byte (one channel, bit depth 1, 2 or 4: the mask files) has the BYTE as its filter
// unit: a "pixel" of the skew is then one byte of the packed row, and each reconstructed byte leaves as its 8 / depth samples,
// scaled, pixels at or behind the width dropped (unpack_byte of csrc/png_inflate_core.h, which the host emulation runs too).
// A stream whose status is not zero is left alone; a filter byte above 4 sets PGDVS_PNG_FILTER.
// Loop bounds are launch arguments; plain byte loads and stores; the one atomic is the status word's OR.
#include "common.h"
#include "png_inflate_core.h"
#include "wave.h"

namespace pgdvs {
namespace {

namespace pi = pnginf;
constexpr int kGroup = 8;  // steps whose loads are issued together

__global__ void __launch_bounds__(kWave) png_unfilter_kernel(const pi::Table table, uint8_t *workspace, uint32_t *__restrict__ status,
                                                             int max_row_blocks, int max_width) {
  const int i = blockIdx.x, lane = threadIdx.x;
  if (__hip_atomic_load(status + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) return;  // (the whole wavefront)
  const pi::Image st = pi::at(table, i);
  const uint8_t *rows = workspace + pi::work_offset(table, i);
  uint8_t *above = workspace + pi::carry_offset(table, i);  // lane 0's upper row, reconstructed
  const int H = st.height, C = st.channels, OC = st.out_channels, D = st.bit_depth;
  const int W = D == 8 ? st.width : (int)pi::row_bytes(st);  // the row's filter units: pixels, or the bytes of packed samples (C = 1)
  const int64_t pitch = 1 + (int64_t)W * C;
  uint8_t *dst = reinterpret_cast<uint8_t *>(st.out);
  bool bad = false;
  for (int rb = 0; rb < max_row_blocks; ++rb) {
    const int base = rb * kWave;
    if (base >= H) break;
    const int y = base + lane;
    const bool valid = y < H;
    const uint8_t *row = rows + (int64_t)(valid ? y : H - 1) * pitch;
    uint32_t ft = row[0];
    if (ft > 4) bad = bad || valid, ft = 0;
    uint8_t *o = dst + (int64_t)(valid ? y : H - 1) * st.row_stride;
    uint32_t cur = 0, up_before = 0;  // the pixel this lane finished last; the upper pixel it was handed last
    for (int k0 = 0; k0 < max_width + kWave - 1; k0 += kGroup) {
      if (k0 >= W + kWave - 1) break;
      uint32_t raw[kGroup], upper[kGroup];  // the group's loads first, all in flight together: a step then waits for none
#pragma unroll
      for (int g = 0; g < kGroup; ++g) {
        const int x = k0 + g - lane;
        raw[g] = 0, upper[g] = 0;
        if (valid && x >= 0 && x < W) {
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            if (c < C) raw[g] |= (uint32_t)row[1 + (int64_t)x * C + c] << (8 * c);
            if (c < C && lane == 0 && base > 0) upper[g] |= (uint32_t)above[(int64_t)x * C + c] << (8 * c);
          }
        }
      }
#pragma unroll
      for (int g = 0; g < kGroup; ++g) {
        uint32_t up = wave_prev_lane(cur);
        const int x = k0 + g - lane;
        if (lane == 0) up = upper[g];
        if (valid && x >= 0 && x < W) {
          if (x == 0) cur = 0, up_before = 0;
          uint32_t px = 0;
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            if (c < C) {
              const uint32_t v = pi::unfilter_byte(ft, (raw[g] >> (8 * c)) & 255, (cur >> (8 * c)) & 255, (up >> (8 * c)) & 255, (up_before >> (8 * c)) & 255);
              px |= v << (8 * c);
              if (lane == kWave - 1) above[(int64_t)x * C + c] = (uint8_t)v;  // the next row block's upper row
              if (D < 8) pi::unpack_byte(v, D, (uint32_t)st.scale, x, st.width, o);
              else if (c < OC) o[(int64_t)x * OC + c] = (uint8_t)v;
            }
          }
          cur = px, up_before = up;
        }
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");  // lane 63's row, then lane 0's loads of it
    __syncthreads();
  }
  if (bad) atomicOr(status + i, pi::kStFilter);
}

}  // namespace

int png_unfilter_launch(const pnginf::Table &table, uint8_t *workspace, uint32_t *status, int max_rows, int max_width, hipStream_t st) {
  PGDVS_LAUNCH("png_unfilter", png_unfilter_kernel, dim3((unsigned)table.n), dim3(kWave), 0, st, table, workspace, status,
               (max_rows + kWave - 1) / kWave, max_width);
  return PGDVS_OK;
}

}  // namespace pgdvs
