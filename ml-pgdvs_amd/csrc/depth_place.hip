// pgdvs_depth_place (include/pgdvs_hip.h states the contract): the float32 payloads of a batch of depth files, as stored,
// into the frames' slots of the resident store -- copied, as 1 / (x + 1e-8), or times a scale -- bit for bit the loaders' numpy
// statements.  One launch: grid.y is the entry, grid.x the blocks of the batch's largest entry (the loaders' frames have one
// size, so the grid is the data); a block whose share lies behind its entry's end does nothing.  Pure streaming, 4 bytes in
// and 4 out per pixel: no LDS, no atomics, no workspace, nothing to report.
//   unmapped  (map == nullptr: the file has the slot's size) an output with contiguous rows is one run of H W floats, any other
//             a run per row.  Where a run's source and destination addresses are equal modulo 16 the run is up to three
//             scalar elements to the boundary, then 16-byte loads and stores, 16 bytes per lane and trip, then a scalar tail;
//             where they differ every element is scalar.
//   mapped    (a NEAREST resize's picks) a thread per output pixel: the map's entry (coalesced), the picked source float,
//             one store.  An entry outside the source reads as 0.
// Arithmetic: the library is built with -ffp-contract=off -fno-fast-math, so the add, the multiply and the divide below are
// each one correctly rounded float32 operation, denormals kept, as numpy's.
#include "common.h"

namespace pgdvs {
namespace {

typedef pgdvs_depth_entry Entry;
constexpr int kBlock = 256;
constexpr unsigned kMaxBlocks = 2048;  // per entry: 8 per CU; larger entries stride

__device__ __forceinline__ float apply(float x, int op, float scale) {
  if (op == PGDVS_DEPTH_RECIPROCAL) return 1.0f / (x + 1e-8f);  // NumPy 2: the weak Python scalars are float32
  if (op == PGDVS_DEPTH_SCALE) return x * scale;
  return x;
}

// one run of n floats, shared by `threads` threads of which this is thread t
__device__ __forceinline__ void run(const float *__restrict__ src, float *__restrict__ out, int64_t n, int64_t t, int64_t threads, int op, float scale) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(src), b = reinterpret_cast<uintptr_t>(out);
  int64_t head = 0, quads = 0;
  if ((a & 15) == (b & 15)) {
    head = (int64_t)(((16 - (a & 15)) & 15) >> 2);
    head = head < n ? head : n;
    quads = (n - head) >> 2;
  }
  const float4 *__restrict__ s4 = reinterpret_cast<const float4 *>(src + head);
  float4 *__restrict__ o4 = reinterpret_cast<float4 *>(out + head);
  for (int64_t q = t; q < quads; q += threads) {
    const float4 x = s4[q];
    o4[q] = make_float4(apply(x.x, op, scale), apply(x.y, op, scale), apply(x.z, op, scale), apply(x.w, op, scale));
  }
  const int64_t body = head + (quads << 2);  // the scalar elements: [0, head) and [body, n)
  for (int64_t i = t; i < head + (n - body); i += threads) {
    const int64_t k = i < head ? i : body + (i - head);
    out[k] = apply(src[k], op, scale);
  }
}

__global__ void __launch_bounds__(kBlock) depth_place_kernel(const Entry *__restrict__ table, const uint8_t *__restrict__ batch) {
  const Entry e = table[blockIdx.y];
  const float *__restrict__ src = reinterpret_cast<const float *>(batch + e.offset);
  uint8_t *__restrict__ out = static_cast<uint8_t *>(e.out);
  const int64_t n = (int64_t)e.H * e.W;
  if (e.map != nullptr) {
    const int64_t hw = (int64_t)e.h * e.w;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
      const int32_t k = e.map[i];
      const float x = k >= 0 && (int64_t)k < hw ? src[k] : 0.0f;
      const int64_t y = i / e.W;
      reinterpret_cast<float *>(out + y * e.out_row_stride)[i - y * e.W] = apply(x, e.op, e.scale);
    }
  } else if (e.out_row_stride == (int64_t)e.W * 4 || e.H == 1) {
    run(src, reinterpret_cast<float *>(out), n, (int64_t)blockIdx.x * kBlock + threadIdx.x, (int64_t)gridDim.x * kBlock, e.op, e.scale);
  } else {
    for (int64_t y = blockIdx.x; y < e.H; y += gridDim.x)
      run(src + y * e.W, reinterpret_cast<float *>(out + y * e.out_row_stride), e.W, threadIdx.x, kBlock, e.op, e.scale);
  }
}

// the blocks an entry asks for: its quads (unmapped and contiguous), its rows (unmapped, rows apart) or its pixels (mapped)
unsigned blocks_of(const Entry &e) {
  const int64_t n = (int64_t)e.H * e.W;
  int64_t want;
  if (e.map != nullptr)
    want = cdiv(n, kBlock);
  else if (e.out_row_stride == (int64_t)e.W * 4 || e.H == 1)
    want = cdiv(cdiv(n, 4) + 3, kBlock);
  else
    want = e.H;
  return (unsigned)(want < (int64_t)kMaxBlocks ? want : (int64_t)kMaxBlocks);
}

}  // namespace
}  // namespace pgdvs

using namespace pgdvs;

PGDVS_API int pgdvs_depth_place(const void *batch_host, const void *batch, int64_t batch_bytes, int32_t n, pgdvs_stream_t stream) {
  const char *op = "pgdvs_depth_place";
  PGDVS_REQUIRE(batch_host && batch, "%s: null pointer", op);
  PGDVS_REQUIRE(n >= 1 && n <= PGDVS_DEPTH_MAX_ENTRIES, "%s: %d entries (1 .. %d)", op, n, PGDVS_DEPTH_MAX_ENTRIES);
  const int64_t table_bytes = align_up((int64_t)n * (int64_t)sizeof(Entry), 16);
  PGDVS_REQUIRE(batch_bytes >= table_bytes, "%s: the batch buffer is shorter than its table", op);
  PGDVS_REQUIRE((reinterpret_cast<uintptr_t>(batch) & 15) == 0, "%s: the batch buffer must be 16-byte aligned", op);
  const Entry *table = static_cast<const Entry *>(batch_host);
  unsigned blocks = 1;
  for (int32_t i = 0; i < n; ++i) {
    const Entry &e = table[i];
    PGDVS_REQUIRE(e.h >= 1 && e.w >= 1 && e.H >= 1 && e.W >= 1 && e.h <= 16384 && e.w <= 16384 && e.H <= 16384 && e.W <= 16384,
                  "%s: entry %d: sizes of 1 .. 16384 expected, got %d x %d -> %d x %d", op, i, e.h, e.w, e.H, e.W);
    PGDVS_REQUIRE(e.op == PGDVS_DEPTH_COPY || e.op == PGDVS_DEPTH_RECIPROCAL || e.op == PGDVS_DEPTH_SCALE, "%s: entry %d: op %d", op, i, e.op);
    PGDVS_REQUIRE(e.offset % 4 == 0, "%s: entry %d: the payload's offset %lld is no multiple of 4", op, i, (long long)e.offset);
    PGDVS_REQUIRE(e.offset >= table_bytes && e.offset <= batch_bytes && (int64_t)e.h * e.w * 4 <= batch_bytes - e.offset,
                  "%s: entry %d: the payload of %d x %d floats at %lld lies outside the buffer's %lld bytes behind the table", op, i, e.h, e.w,
                  (long long)e.offset, (long long)batch_bytes);
    PGDVS_REQUIRE(e.map != nullptr || (e.H == e.h && e.W == e.w), "%s: entry %d: without a map the sizes are equal", op, i);
    PGDVS_REQUIRE((reinterpret_cast<uintptr_t>(e.map) & 3) == 0, "%s: entry %d: map must be 4-byte aligned", op, i);
    PGDVS_REQUIRE(e.out != nullptr && (reinterpret_cast<uintptr_t>(e.out) & 3) == 0 && e.out_row_stride >= (int64_t)e.W * 4 && e.out_row_stride % 4 == 0,
                  "%s: entry %d: out is 4-byte aligned, its row stride at least 4 W bytes and a multiple of 4", op, i);
    const unsigned b = blocks_of(e);
    blocks = b > blocks ? b : blocks;
  }
  PGDVS_LAUNCH("depth_place", depth_place_kernel, dim3(blocks, (unsigned)n), dim3(kBlock), 0, as_stream(stream), static_cast<const Entry *>(batch),
               static_cast<const uint8_t *>(batch));
  return check_launch(op);
}
