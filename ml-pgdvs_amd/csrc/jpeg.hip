// The visualiser's video (pgdvs/engines/visualizer_pgdvs.py:141-177, pgdvs/utils/rendering.py:79-116 images_to_video): the frames
// of <scene_id>_combined.avi leave the GPU as baseline JPEG scan data.  Upstream pipes PNG-sized frames into ffmpeg (H.264 in
// an mp4); here every frame is an independent JPEG -- 8 bit, Y Cb Cr 4:4:4, one interleaved scan, the four standard Huffman
// tables -- and pgdvs_amd/video.py owns the headers and the AVI container, as png.py owns the PNG container.  The codec is
// stated in integers (video.py holds the same statement in numpy), so host and device agree byte for byte.
//
// pgdvs_jpeg_coefficients: one wavefront per MCU (an 8 x 8 pixel block of Y, Cb, Cr), lane = pixel.  A lane quantises its
// pixel as *_combined.png does, converts it with JFIF's 16-bit fixed point and takes part in the two DCT passes through LDS:
// the 13-bit integer DCT of Loeffler, Ligtenberg and Moschytz in the Independent JPEG Group's scaling, rows then columns, whose
// result is 8 x the coefficient (fdct_1d; every lane computes its row's / column's eight outputs and keeps its own); then it
// quantises the coefficient it holds with ONE rounding, sign(c) ((|c| + 4 Q) / (8 Q)), and the block leaves in zigzag order
// as 32 dword stores.  These are libjpeg's coefficients: PIL writes the same scan bytes at the same tables and 4:4:4.
//
// pgdvs_jpeg_scan: three launches, no workgroup waits for another, every loop bound is known at launch.
//   1 jpeg_segments  one workgroup of 256 threads per restart segment, thread = block (Y, Cb, Cr of MCU 0, then MCU 1, ...),
//                    256 blocks at a time.  A thread walks its 64 coefficients for the bit length, the block-wide scan gives
//                    its bit offset, a second walk ORs the codes into an LDS bit buffer (a word at a time: only words shared
//                    with a neighbour see more than one atomic).  The whole bytes of the buffer are then stuffed (0xFF ->
//                    0xFF 0x00; a word per thread, a second scan for the byte offsets) into the segment's fixed-stride slot;
//                    the 0 .. 7 bits left over open the next 256 blocks' buffer, and the last ones are padded with ones.
//   2 jpeg_offsets   one workgroup per frame scans the segment sizes (plus two bytes per RSTm marker) into byte offsets and
//                    writes the frame's length.
//   3 jpeg_gather    one workgroup per segment copies its slot to its offset in the frame's contiguous stream and appends
//                    the marker.
// The coefficients are read twice (the second time from the cache) rather than kept as codes in LDS: a block's codes can take
// 1658 bits, 256 of them more than the bit buffer itself.
//
// pgdvs_jpeg_coefficients_420 / pgdvs_jpeg_scan_420: the same codec at 4:2:0, upstream's chroma format (its ffmpeg writer's
// yuv420p): MCUs of 16 x 16 pixels and six blocks, Y00 Y01 Y10 Y11 Cb Cr, with libjpeg's 2 x 2 chroma average, edge rules and
// dummy blocks (jpeg_coefficients_420_kernel), and the entropy coder above with six blocks per MCU (jpeg_segments_kernel<6>).
#include "common.h"
#include "quant8.h"
#include "wave.h"

namespace pgdvs {
namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / kWave;

// ---- tables ------------------------------------------------------------------------------------------------------------------
// rint(8192 x) of the DCT's twelve constants (tests/test_video_host.py reads these lines and compares them with video.py's)
constexpr int kFix_0_298631336 = 2446, kFix_0_390180644 = 3196, kFix_0_541196100 = 4433, kFix_0_765366865 = 6270;
constexpr int kFix_0_899976223 = 7373, kFix_1_175875602 = 9633, kFix_1_501321110 = 12299, kFix_1_847759065 = 15137;
constexpr int kFix_1_961570560 = 16069, kFix_2_053119869 = 16819, kFix_2_562915447 = 20995, kFix_3_072711026 = 25172;
constexpr int kDctBits = 13, kPass1Bits = 2;

// position in the zigzag sequence of the coefficient at natural (row-major) index i
__device__ const uint8_t kZigzagPos[64] = {0,  1,  5,  6,  14, 15, 27, 28, 2,  4,  7,  13, 16, 26, 29, 42, 3,  8,  12, 17, 25, 30,
                                           41, 43, 9,  11, 18, 24, 31, 40, 44, 53, 10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38,
                                           46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63};

// ITU-T T.81 Annex K.3, the four typical Huffman tables as BITS / HUFFVAL; expanded at compile time to code | length << 16
// per symbol (Annex C).  A symbol the tables do not hold has length 0; the clamps below keep every look-up on a held one.
struct HuffSpec {
  uint8_t bits[16];
  uint8_t vals[162];
};
constexpr HuffSpec kDcLuma = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}};
constexpr HuffSpec kDcChroma = {{0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}};
constexpr HuffSpec kAcLuma = {
    {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125},
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
     0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18,
     0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
     0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75,
     0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
     0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
     0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5,
     0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}};
constexpr HuffSpec kAcChroma = {
    {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08,
     0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25,
     0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47,
     0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74,
     0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97,
     0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
     0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4,
     0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}};

// [0] luminance, [1] chrominance; AC indexed by run << 4 | size, DC by size
struct HuffTables {
  uint32_t ac[2][256];
  uint32_t dc[2][16];
};
constexpr void expand(const HuffSpec &s, uint32_t *out) {
  uint32_t code = 0;
  int k = 0;
  for (int len = 1; len <= 16; ++len) {
    for (int i = 0; i < s.bits[len - 1]; ++i, ++k, ++code) out[s.vals[k]] = code | ((uint32_t)len << 16);
    code <<= 1;
  }
}
constexpr HuffTables make_tables() {
  HuffTables t{};
  expand(kAcLuma, t.ac[0]);
  expand(kAcChroma, t.ac[1]);
  expand(kDcLuma, t.dc[0]);
  expand(kDcChroma, t.dc[1]);
  return t;
}
__device__ const HuffTables kHuff = make_tables();
constexpr int kHuffWords = sizeof(HuffTables) / 4;

constexpr int kDcMin = -1024, kDcMax = 1023, kAcMax = 1023;
constexpr int kBlockMaxBits = 20 + 63 * 26;                    // 1658: DC 9 + 11, every AC 16 + 10
constexpr int kBlockMaxBytes = 2 * ((kBlockMaxBits + 7) / 8);  // 416: every byte stuffed

// ---- coefficients ----------------------------------------------------------------------------------------------------------------
// Both kernels quantise the pixels as *_combined.png is (quant8.h's quantise_save_image) and take these parameters.
struct CoefParams {
  const float *img;    // [B,3,H,W]
  int16_t *coef;       // [B,nmy,nmx,3 or 6,64]
  int H, W, nmy, nmx;  // the MCU grid: 8 x 8 pixels an MCU at 4:4:4, 16 x 16 at 4:2:0
  int nby, nbx;        // ceil(H / 8), ceil(W / 8): at 4:4:4 the MCU grid again; at 4:2:0 luma blocks past them are dummies
  int n_mcu;           // B nmy nmx
  uint16_t q[2][64];   // natural order
};

__device__ __forceinline__ int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// One pass of the DCT over d[0..7] -> output k.  kFirst: the row pass, whose results stay scaled up by 2^kPass1Bits; the column
// pass takes that scale out again, but for a factor of 8 overall.  All sums fit int32 (|d| <= 128, then <= 2^13).
template <bool kFirst>
__device__ __forceinline__ int fdct_1d(const int *d, int k) {
  int t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6];
  int t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
  const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  constexpr int n = kFirst ? kDctBits - kPass1Bits : kDctBits + kPass1Bits;
  int o[8];
  o[0] = kFirst ? (t10 + t11) << kPass1Bits : descale(t10 + t11, kPass1Bits);
  o[4] = kFirst ? (t10 - t11) << kPass1Bits : descale(t10 - t11, kPass1Bits);
  int z1 = (t12 + t13) * kFix_0_541196100;
  o[2] = descale(z1 + t13 * kFix_0_765366865, n);
  o[6] = descale(z1 - t12 * kFix_1_847759065, n);
  z1 = t4 + t7;
  int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
  const int z5 = (z3 + z4) * kFix_1_175875602;
  t4 *= kFix_0_298631336;
  t5 *= kFix_2_053119869;
  t6 *= kFix_3_072711026;
  t7 *= kFix_1_501321110;
  z1 *= -kFix_0_899976223;
  z2 *= -kFix_2_562915447;
  z3 = z5 - z3 * kFix_1_961570560;
  z4 = z5 - z4 * kFix_0_390180644;
  o[7] = descale(t4 + z1 + z3, n);
  o[5] = descale(t5 + z2 + z4, n);
  o[3] = descale(t6 + z2 + z3, n);
  o[1] = descale(t7 + z1 + z4, n);
  int r = o[0];
#pragma unroll
  for (int i = 1; i < 8; ++i) r = k == i ? o[i] : r;
  return r;
}

// One 8 x 8 block of a wavefront: the lane's level-shifted sample -> the quantised coefficient at the lane's natural index
// (vertical frequency r = lane >> 3, horizontal c = lane & 7).  a, b: the wavefront's 64 words of LDS each; q: the table in LDS.
// Holds two workgroup barriers (the first also orders the tables' staging before their first use).
__device__ __forceinline__ int block_coefficient(int sample, int *a, int *b, const int *q, int lane, int r, int c) {
  a[lane] = sample;
  __syncthreads();
  int d[8];
#pragma unroll
  for (int n = 0; n < 8; ++n) d[n] = a[r * 8 + n];
  b[lane] = fdct_1d<true>(d, c);  // row r, horizontal frequency c
  __syncthreads();
#pragma unroll
  for (int n = 0; n < 8; ++n) d[n] = b[n * 8 + c];
  const int u = fdct_1d<false>(d, r);  // vertical frequency r, horizontal frequency c, times 8
  const int Q8 = q[lane] << 3;
  const int mag = (abs(u) + (Q8 >> 1)) / Q8;
  return u < 0 ? -mag : mag;
}

__global__ void __launch_bounds__(kBlock) jpeg_coefficients_kernel(CoefParams p) {
  __shared__ int s_q[2][64];
  __shared__ int s_a[kWaves][64];
  __shared__ int s_b[kWaves][64];
  __shared__ __attribute__((aligned(16))) int16_t s_zz[kWaves][64];
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  if (threadIdx.x < 128) s_q[threadIdx.x >> 6][threadIdx.x & 63] = p.q[threadIdx.x >> 6][threadIdx.x & 63];
  // a wavefront past the last MCU redoes the last one and stores nothing: every barrier below is met by all four
  const int mcu_raw = blockIdx.x * kWaves + wave;
  const bool live = mcu_raw < p.n_mcu;
  const int mcu = live ? mcu_raw : p.n_mcu - 1;
  const int per = p.nby * p.nbx;
  const int b = mcu / per, rem = mcu - b * per;
  const int by = rem / p.nbx, bx = rem - by * p.nbx;
  const int r = lane >> 3, c = lane & 7;
  const int y = min(by * 8 + r, p.H - 1), x = min(bx * 8 + c, p.W - 1);  // libjpeg's edge expansion
  const size_t plane = (size_t)p.H * p.W;
  const float *px = p.img + (size_t)b * 3 * plane + (size_t)y * p.W + x;
  const int R = quantise_save_image(px[0]), G = quantise_save_image(px[plane]), B = quantise_save_image(px[2 * plane]);
  int s[3];
  s[0] = ((19595 * R + 38470 * G + 7471 * B + 32768) >> 16) - 128;
  s[1] = ((-11059 * R - 21709 * G + 32768 * B + 8421375) >> 16) - 128;
  s[2] = ((32768 * R - 27439 * G - 5329 * B + 8421375) >> 16) - 128;
  int16_t *out = p.coef + (size_t)mcu * 3 * 64;
#pragma unroll
  for (int comp = 0; comp < 3; ++comp) {
    s_zz[wave][kZigzagPos[lane]] = (int16_t)block_coefficient(s[comp], s_a[wave], s_b[wave], s_q[comp ? 1 : 0], lane, r, c);
    __syncthreads();
    if (live && lane < 32) reinterpret_cast<uint32_t *>(out + comp * 64)[lane] = reinterpret_cast<const uint32_t *>(s_zz[wave])[lane];
  }
}

// ---- coefficients, 4:2:0 ---------------------------------------------------------------------------------------------------------
// libjpeg's 4:2:0 (include/pgdvs_hip.h states the rules; pgdvs_amd/video.py restates them in numpy): one wavefront per 16 x 16
// MCU, six blocks in the order Y00, Y01, Y10, Y11, Cb, Cr, lane = sample of the current 8 x 8 block, the DCT as above.
// Cb and Cr (0 .. 255) of the pixel at px, packed as Cb | Cr << 16 so that the four of a quad add up in one register
__device__ __forceinline__ int cbcr_packed(const float *px, size_t plane) {
  const int R = quantise_save_image(px[0]), G = quantise_save_image(px[plane]), B = quantise_save_image(px[2 * plane]);
  const int cb = (-11059 * R - 21709 * G + 32768 * B + 8421375) >> 16;
  const int cr = (32768 * R - 27439 * G - 5329 * B + 8421375) >> 16;
  return cb | (cr << 16);
}

__global__ void __launch_bounds__(kBlock) jpeg_coefficients_420_kernel(CoefParams p) {
  __shared__ int s_q[2][64];
  __shared__ int s_a[kWaves][64];
  __shared__ int s_b[kWaves][64];
  __shared__ __attribute__((aligned(16))) int16_t s_zz[kWaves][64];
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  if (threadIdx.x < 128) s_q[threadIdx.x >> 6][threadIdx.x & 63] = p.q[threadIdx.x >> 6][threadIdx.x & 63];
  // a wavefront past the last MCU redoes the last one and stores nothing: every barrier below is met by all four
  const int mcu_raw = blockIdx.x * kWaves + wave;
  const bool live = mcu_raw < p.n_mcu;
  const int mcu = live ? mcu_raw : p.n_mcu - 1;
  const int per = p.nmy * p.nmx;
  const int b = mcu / per, rem = mcu - b * per;
  const int my = rem / p.nmx, mx = rem - my * p.nmx;
  const int r = lane >> 3, c = lane & 7;
  const size_t plane = (size_t)p.H * p.W;
  const float *img = p.img + (size_t)b * 3 * plane;
  // every index below is clamped into the image: the samples of dummy blocks are read and transformed like any others (the
  // wavefronts of a workgroup meet the same barriers) and only their result is replaced
  int s[6];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int y = min((2 * my + (k >> 1)) * 8 + r, p.H - 1), x = min((2 * mx + (k & 1)) * 8 + c, p.W - 1);
    const float *px = img + (size_t)y * p.W + x;
    const int R = quantise_save_image(px[0]), G = quantise_save_image(px[plane]), B = quantise_save_image(px[2 * plane]);
    s[k] = ((19595 * R + 38470 * G + 7471 * B + 32768) >> 16) - 128;
  }
  {
    // chroma sample (j, i) = (8 my + r, 8 mx + c): rows past the last downsampled one repeat it, then the quad's own clamps
    const int j = min(8 * my + r, ((p.H + 1) >> 1) - 1), i = 8 * mx + c;
    const int y0 = min(2 * j, p.H - 1), y1 = min(2 * j + 1, p.H - 1), x0 = min(2 * i, p.W - 1), x1 = min(2 * i + 1, p.W - 1);
    const float *row0 = img + (size_t)y0 * p.W, *row1 = img + (size_t)y1 * p.W;
    const int sum = cbcr_packed(row0 + x0, plane) + cbcr_packed(row0 + x1, plane) + cbcr_packed(row1 + x0, plane) +
                    cbcr_packed(row1 + x1, plane);  // each half at most 1020: no carry between them
    const int bias = 1 + (c & 1);                   // (8 mx is even: the parity of i is that of c)
    s[4] = (((sum & 0xffff) + bias) >> 2) - 128;
    s[5] = (((sum >> 16) + bias) >> 2) - 128;
  }
  const bool right_dummy = 2 * mx + 1 >= p.nbx, bottom_dummy = 2 * my + 1 >= p.nby;
  int16_t *out = p.coef + (size_t)mcu * 6 * 64;
  int dc[3];  // the quantised DC of Y00, Y01, Y10 as stored (wavefront-uniform)
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    int v = block_coefficient(s[k], s_a[wave], s_b[wave], s_q[k < 4 ? 0 : 1], lane, r, c);
    // dummy blocks: no AC, the DC of Y01 for the bottom row (which wins), of the left neighbour for the right column
    if (k == 1 && right_dummy) v = lane == 0 ? dc[0] : 0;
    if (k == 2 && bottom_dummy) v = lane == 0 ? dc[1] : 0;
    if (k == 3 && (bottom_dummy || right_dummy)) v = lane == 0 ? (bottom_dummy ? dc[1] : dc[2]) : 0;
    if (k < 3) dc[k] = __builtin_amdgcn_readfirstlane(v);  // lane 0 holds natural index 0
    s_zz[wave][kZigzagPos[lane]] = (int16_t)v;
    __syncthreads();
    if (live && lane < 32) reinterpret_cast<uint32_t *>(out + k * 64)[lane] = reinterpret_cast<const uint32_t *>(s_zz[wave])[lane];
  }
}

// ---- entropy coding ----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int size_of(int v) { return 32 - __clz(abs(v)); }  // the JPEG "category": bits of |v|
__device__ __forceinline__ int clamp_dc(int v) { return min(max(v, kDcMin), kDcMax); }
__device__ __forceinline__ int clamp_ac(int v) { return min(max(v, -kAcMax), kAcMax); }

// Walks one block's symbols in stream order and hands each to emit(value, length): the Huffman code with the coefficient's
// bits behind it, at most 26 bits.  huff: the tables in LDS; t: 0 luminance, 1 chrominance.
template <class Emit>
__device__ __forceinline__ void walk_block(const int16_t *__restrict__ blk, int pred, const HuffTables &huff, int t, Emit &&emit) {
  int run = 0;
  for (int q = 0; q < 8; ++q) {
    const uint4 w = reinterpret_cast<const uint4 *>(blk)[q];
    const uint32_t ws[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int raw = (int)(int16_t)(ws[i >> 1] >> (16 * (i & 1)));
      if (q == 0 && i == 0) {
        const int d = clamp_dc(raw) - pred;
        const int n = size_of(d);
        const uint32_t h = huff.dc[t][n];
        emit(((h & 0xffffu) << n) | (uint32_t)(d >= 0 ? d : d + (1 << n) - 1), (int)(h >> 16) + n);
        continue;
      }
      const int v = clamp_ac(raw);
      if (v == 0) {
        ++run;
        continue;
      }
      const uint32_t zrl = huff.ac[t][0xF0];
      for (int z = 0; z < 3; ++z)  // (a run is at most 62)
        if (run > 15) {
          emit(zrl & 0xffffu, (int)(zrl >> 16));
          run -= 16;
        }
      const int n = size_of(v);
      const uint32_t h = huff.ac[t][(run << 4) | n];
      emit(((h & 0xffffu) << n) | (uint32_t)(v >= 0 ? v : v + (1 << n) - 1), (int)(h >> 16) + n);
      run = 0;
    }
  }
  if (run > 0) {
    const uint32_t eob = huff.ac[t][0];
    emit(eob & 0xffffu, (int)(eob >> 16));
  }
}

constexpr int kBufWords = (7 + kBlock * kBlockMaxBits + 31) / 32 + 2;  // + the word a code may spill into, never past it

struct ScanParams {
  const int16_t *coef;  // [B,n_mcu,kBpm,64]
  int n_mcu;            // per frame
  int seg_mcus;         // MCUs per restart segment (>= 1)
  int n_seg;            // per frame
  uint8_t *slots;       // [B n_seg][slot_stride]
  int64_t slot_stride;
  uint32_t *sizes;      // [B n_seg] stuffed bytes per segment
  uint32_t *offsets;    // [B n_seg] byte offset of the segment in its frame's stream
  uint8_t *out;
  int64_t out_stride;
  int32_t *nbytes;      // [B]
};

// bits are big-endian throughout: bit 0 of the buffer is the most significant bit of word 0, byte i of the buffer is bits
// 31 - 8 (i & 3) .. 24 - 8 (i & 3) of word i >> 2.
// kBpm: blocks per MCU.  3: Y Cb Cr, each predicted from the block 3 back.  6 (4:2:0): Y00 Y01 Y10 Y11 Cb Cr; the previous
// block of the component is 3 back for Y00 (the Y11 of the MCU before), 1 back for Y01 .. Y11, 6 back for Cb and Cr.
template <int kBpm>
__global__ void __launch_bounds__(kBlock) jpeg_segments_kernel(ScanParams p) {
  static_assert(kBpm == 3 || kBpm == 6, "4:4:4 or 4:2:0");
  __shared__ HuffTables s_huff;
  __shared__ uint32_t s_buf[kBufWords];
  __shared__ int s_wsum[kWaves];
  const int tid = threadIdx.x;
  for (int i = tid; i < kHuffWords; i += kBlock) reinterpret_cast<uint32_t *>(&s_huff)[i] = reinterpret_cast<const uint32_t *>(&kHuff)[i];
  const int frame = blockIdx.x / p.n_seg, seg = blockIdx.x - frame * p.n_seg;
  const int mcu0 = seg * p.seg_mcus;
  const int n_blk = kBpm * min(p.seg_mcus, p.n_mcu - mcu0);  // blocks of this segment
  const int16_t *blocks = p.coef + ((size_t)frame * p.n_mcu + mcu0) * kBpm * 64;
  uint8_t *slot = p.slots + (size_t)blockIdx.x * p.slot_stride;
  uint32_t carry = 0u;  // the bits left over by the blocks before, left-aligned in a byte
  int n_carry = 0;
  uint32_t written = 0u;
  __syncthreads();
  for (int j0 = 0; j0 < n_blk; j0 += kBlock) {
    const int j = j0 + tid;
    const bool have = j < n_blk;
    const int16_t *blk = blocks + (size_t)(have ? j : 0) * 64;
    const int at = j % kBpm;  // the block's place in its MCU
    const int t = at >= (kBpm == 3 ? 1 : 4) ? 1 : 0;
    const int back = kBpm == 3 ? 3 : (at == 0 ? 3 : at < 4 ? 1 : 6);
    // the first block of a component in the segment predicts from 0 (those 1 back always have a block in front of them)
    const int pred = (have && (back == 1 || j >= kBpm)) ? clamp_dc((int)blk[-back * 64]) : 0;
    int len = 0;
    if (have) walk_block(blk, pred, s_huff, t, [&](uint32_t, int n) { len += n; });
    int total;
    const int pos0 = n_carry + block_excl_scan<kWaves>(len, s_wsum, total);
    total += n_carry;
    const bool last = j0 + kBlock >= n_blk;
    const int n_bits = last ? (total + 7) & ~7 : total;  // the segment ends on a byte, padded with ones
    for (int w = tid; w <= (n_bits >> 5) + 1; w += kBlock) s_buf[w] = w == 0 ? carry << 24 : 0u;
    __syncthreads();
    if (have) {
      int pos = pos0, w = pos0 >> 5;
      uint32_t cur = 0u;
      walk_block(blk, pred, s_huff, t, [&](uint32_t v, int n) {
        const uint64_t x = (uint64_t)v << (64 - n - (pos & 31));
        cur |= (uint32_t)(x >> 32);
        pos += n;
        if ((pos >> 5) != w) {
          atomicOr(&s_buf[w], cur);
          ++w;
          cur = (uint32_t)x;
        }
      });
      if (cur) atomicOr(&s_buf[w], cur);
    }
    if (tid == 0 && n_bits != total) atomicOr(&s_buf[total >> 5], (0xffffffffu >> (total & 31)) & ~(0xffffffffu >> 1 >> ((n_bits - 1) & 31)));
    __syncthreads();
    // whole bytes out, a word per thread
    const int n_bytes = n_bits >> 3;
    for (int w0 = 0; w0 * 4 < n_bytes; w0 += kBlock) {
      const int w = w0 + tid;
      const int nb = min(max(n_bytes - 4 * w, 0), 4);
      const uint32_t word = nb > 0 ? s_buf[w] : 0u;
      int ff = 0;
#pragma unroll
      for (int i = 0; i < 4; ++i) ff += (i < nb && ((word >> (24 - 8 * i)) & 255u) == 255u) ? 1 : 0;
      int all;
      uint32_t at = written + (uint32_t)block_excl_scan<kWaves>(nb + ff, s_wsum, all);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (i < nb) {
          const uint32_t byte = (word >> (24 - 8 * i)) & 255u;
          slot[at++] = (uint8_t)byte;
          if (byte == 255u) slot[at++] = 0;
        }
      }
      written += (uint32_t)all;
      __syncthreads();  // s_wsum is written again
    }
    n_carry = n_bits & 7;
    carry = n_carry ? (s_buf[n_bytes >> 2] >> (24 - 8 * (n_bytes & 3))) & 255u : 0u;
    __syncthreads();  // every thread holds the carry before the buffer is cleared
  }
  if (tid == 0) p.sizes[blockIdx.x] = written;
}

// segment s of a frame lies at sum over s' < s of (sizes[s'] + 2): the marker behind every segment but the last
__global__ void __launch_bounds__(kBlock) jpeg_offsets_kernel(ScanParams p) {
  __shared__ int s_wsum[kWaves];
  const int frame = blockIdx.x;
  const uint32_t *sizes = p.sizes + (size_t)frame * p.n_seg;
  uint32_t *offsets = p.offsets + (size_t)frame * p.n_seg;
  int base = 0;
  for (int s0 = 0; s0 < p.n_seg; s0 += kBlock) {
    const int s = s0 + (int)threadIdx.x;
    const int c = s < p.n_seg ? (int)sizes[s] + (s + 1 < p.n_seg ? 2 : 0) : 0;
    int total;
    const int off = base + block_excl_scan<kWaves>(c, s_wsum, total);
    if (s < p.n_seg) offsets[s] = (uint32_t)off;
    base += total;
    __syncthreads();
  }
  if (threadIdx.x == 0) p.nbytes[frame] = base;
}

__global__ void __launch_bounds__(kBlock) jpeg_gather_kernel(ScanParams p) {
  const int frame = blockIdx.x / p.n_seg, seg = blockIdx.x - frame * p.n_seg;
  const uint8_t *slot = p.slots + (size_t)blockIdx.x * p.slot_stride;
  const uint32_t n = p.sizes[blockIdx.x];
  uint8_t *dst = p.out + (size_t)frame * p.out_stride + p.offsets[blockIdx.x];
  for (uint32_t i = threadIdx.x; i < n; i += kBlock) dst[i] = slot[i];
  if (threadIdx.x == 0 && seg + 1 < p.n_seg) {
    dst[n] = 0xFF;
    dst[n + 1] = (uint8_t)(0xD0 + (seg & 7));
  }
}

// Shapes of a scan call -> segments per frame, MCUs per segment, slot stride, capacity of a frame's stream; false if invalid
struct ScanShape {
  int64_t n_mcu, seg_mcus, n_seg, slot_stride, capacity;
};
// nby, nbx: the MCU grid (16 x 16 pixel MCUs at bpm = 6), at most grid_side a side: either way no more than 65536 pixels
constexpr int grid_side(int bpm) { return bpm == 3 ? 8192 : 4096; }
bool scan_shape(int B, int nby, int nbx, int restart_mcus, int bpm, ScanShape &s) {
  const int side = grid_side(bpm);
  if (B < 1 || nby < 1 || nby > side || nbx < 1 || nbx > side || restart_mcus < 1 || restart_mcus > 65535) return false;
  s.n_mcu = (int64_t)nby * nbx;
  s.seg_mcus = restart_mcus < s.n_mcu ? restart_mcus : s.n_mcu;
  s.n_seg = cdiv(s.n_mcu, s.seg_mcus);
  s.slot_stride = s.seg_mcus * bpm * kBlockMaxBytes;
  s.capacity = s.n_mcu * bpm * kBlockMaxBytes + 2 * (s.n_seg - 1);
  return (int64_t)B * s.n_seg * s.slot_stride < (1ll << 31) && (int64_t)B * s.capacity < (1ll << 31);
}

struct ScanWorkspace {
  uint32_t *sizes, *offsets;
  uint8_t *slots;
  int64_t bytes;
  ScanWorkspace(void *base, int B, const ScanShape &s) {
    Carver c{static_cast<char *>(base)};
    sizes = c.take<uint32_t>(B * s.n_seg * 4);
    offsets = c.take<uint32_t>(B * s.n_seg * 4);
    slots = c.take<uint8_t>(B * s.n_seg * s.slot_stride);
    bytes = c.off;
  }
};

// the three launches of a scan over checked shapes
template <int kBpm>
void launch_scan(const int16_t *coef, int B, const ScanShape &s, const ScanWorkspace &ws, uint8_t *out, int64_t out_stride,
                 int32_t *nbytes, hipStream_t st) {
  ScanParams p;
  p.coef = coef;
  p.n_mcu = (int)s.n_mcu;
  p.seg_mcus = (int)s.seg_mcus;
  p.n_seg = (int)s.n_seg;
  p.slots = ws.slots;
  p.slot_stride = s.slot_stride;
  p.sizes = ws.sizes;
  p.offsets = ws.offsets;
  p.out = out;
  p.out_stride = out_stride;
  p.nbytes = nbytes;
  const unsigned n_slots = (unsigned)(B * s.n_seg);
  PGDVS_LAUNCH("jpeg_segments", jpeg_segments_kernel<kBpm>, dim3(n_slots), dim3(kBlock), 0, st, p);
  PGDVS_LAUNCH("jpeg_offsets", jpeg_offsets_kernel, dim3((unsigned)B), dim3(kBlock), 0, st, p);
  PGDVS_LAUNCH("jpeg_gather", jpeg_gather_kernel, dim3(n_slots), dim3(kBlock), 0, st, p);
}

// ---- the entry points' bodies, per blocks of an MCU (3: 4:4:4, 8 x 8 MCUs; 6: 4:2:0, 16 x 16); fn: the entry point, for the messages ----
int coefficients(const char *fn, int bpm, const float *img_planar, int B, int H, int W, const uint16_t *qtab_luma,
                 const uint16_t *qtab_chroma, int16_t *coef, hipStream_t st) {
  PGDVS_REQUIRE(img_planar && qtab_luma && qtab_chroma && coef, "%s: null pointer", fn);
  PGDVS_REQUIRE(B >= 1 && H >= 1 && H <= 65535 && W >= 1 && W <= 65535, "%s: bad shape B=%d H=%d W=%d (B >= 1, H and W in 1 .. 65535)", fn,
                B, H, W);
  const int mcu_px = bpm == 3 ? 8 : 16;
  CoefParams p;
  p.img = img_planar;
  p.coef = coef;
  p.H = H;
  p.W = W;
  p.nmy = (H + mcu_px - 1) / mcu_px;
  p.nmx = (W + mcu_px - 1) / mcu_px;
  p.nby = (H + 7) / 8;
  p.nbx = (W + 7) / 8;
  const int64_t n_coef = (int64_t)B * p.nmy * p.nmx * bpm * 64;
  PGDVS_REQUIRE((int64_t)B * 3 * H * W < (1ll << 31) && n_coef < (1ll << 31),
                "%s: B=%d H=%d W=%d: 3 B H W and the %lld coefficients must stay below 2^31", fn, B, H, W, (long long)n_coef);
  PGDVS_REQUIRE((reinterpret_cast<uintptr_t>(img_planar) & 3) == 0 && (reinterpret_cast<uintptr_t>(coef) & 3) == 0,
                "%s: img_planar or coef is not 4-byte aligned", fn);
  p.n_mcu = B * p.nmy * p.nmx;
  for (int i = 0; i < 64; ++i) {
    PGDVS_REQUIRE(qtab_luma[i] >= 1 && qtab_luma[i] <= 255 && qtab_chroma[i] >= 1 && qtab_chroma[i] <= 255,
                  "%s: quantisation table entry %d is %d / %d (1 .. 255: baseline, 8-bit tables)", fn, i, (int)qtab_luma[i],
                  (int)qtab_chroma[i]);
    p.q[0][i] = qtab_luma[i];
    p.q[1][i] = qtab_chroma[i];
  }
  const dim3 grid((unsigned)cdiv(p.n_mcu, kWaves));
  if (bpm == 3)
    PGDVS_LAUNCH("jpeg_coefficients", jpeg_coefficients_kernel, grid, dim3(kBlock), 0, st, p);
  else
    PGDVS_LAUNCH("jpeg_coefficients_420", jpeg_coefficients_420_kernel, grid, dim3(kBlock), 0, st, p);
  return check_launch(fn);
}

// scan_shape, with the entry point's complaint about a shape it refuses (the grid's names are those of the entry's arguments)
bool checked_scan_shape(const char *fn, int bpm, int B, int ny, int nx, int restart_mcus, ScanShape &s) {
  if (scan_shape(B, ny, nx, restart_mcus, bpm, s)) return true;
  const char *g = bpm == 3 ? "nb" : "nm";
  set_error("%s: bad shape B=%d %sy=%d %sx=%d restart_mcus=%d (B >= 1, %sy and %sx in 1 .. %d, restart_mcus in 1 .. 65535, B x the "
            "frame's capacity below 2^31)", fn, B, g, ny, g, nx, restart_mcus, g, g, grid_side(bpm));
  return false;
}

int64_t scan_workspace_bytes(const char *fn, int bpm, int B, int ny, int nx, int restart_mcus) {
  ScanShape s;
  if (!checked_scan_shape(fn, bpm, B, ny, nx, restart_mcus, s)) return -1;
  return ScanWorkspace(nullptr, B, s).bytes;
}

template <int kBpm>
int scan(const char *fn, const int16_t *coef, int B, int ny, int nx, int restart_mcus, uint8_t *out, int64_t out_stride, int32_t *nbytes,
         void *workspace, int64_t workspace_bytes, hipStream_t st) {
  PGDVS_REQUIRE(coef && out && nbytes && workspace, "%s: null pointer", fn);
  PGDVS_REQUIRE(restart_mcus != 0, "%s: restart_mcus 0 (no restart markers) is host-only: the segments of the device pass are "
                                   "byte-aligned; use 1 .. 65535", fn);
  ScanShape s;
  if (!checked_scan_shape(fn, kBpm, B, ny, nx, restart_mcus, s)) return PGDVS_ERR_INVALID;
  const char *g = kBpm == 3 ? "nb" : "nm";
  PGDVS_REQUIRE(out_stride >= s.capacity && (int64_t)B * out_stride < (1ll << 31),
                "%s: out_stride %lld (at least the capacity %lld = %d %sy %sx + 2 (segments - 1), B out_stride < 2^31)", fn,
                (long long)out_stride, (long long)s.capacity, kBpm * kBlockMaxBytes, g, g);
  PGDVS_REQUIRE((reinterpret_cast<uintptr_t>(coef) & 15) == 0 && (reinterpret_cast<uintptr_t>(workspace) & 255) == 0 &&
                    (reinterpret_cast<uintptr_t>(nbytes) & 3) == 0,
                "%s: coef must be 16-byte, workspace 256-byte and nbytes 4-byte aligned", fn);
  ScanWorkspace ws(workspace, B, s);
  PGDVS_REQUIRE(workspace_bytes >= ws.bytes, "%s: workspace of %lld bytes, %lld needed", fn, (long long)workspace_bytes, (long long)ws.bytes);
  launch_scan<kBpm>(coef, B, s, ws, out, out_stride, nbytes, st);
  return check_launch(fn);
}

}  // namespace
}  // namespace pgdvs

using namespace pgdvs;

PGDVS_API int pgdvs_jpeg_coefficients(const float *img_planar, int B, int H, int W, const uint16_t *qtab_luma, const uint16_t *qtab_chroma,
                                      int16_t *coef, pgdvs_stream_t stream) {
  return coefficients("pgdvs_jpeg_coefficients", 3, img_planar, B, H, W, qtab_luma, qtab_chroma, coef, as_stream(stream));
}

PGDVS_API int64_t pgdvs_jpeg_scan_workspace_bytes(int B, int nby, int nbx, int restart_mcus) {
  return scan_workspace_bytes("pgdvs_jpeg_scan_workspace_bytes", 3, B, nby, nbx, restart_mcus);
}

PGDVS_API int pgdvs_jpeg_scan(const int16_t *coef, int B, int nby, int nbx, int restart_mcus, uint8_t *out, int64_t out_stride,
                              int32_t *nbytes, void *workspace, int64_t workspace_bytes, pgdvs_stream_t stream) {
  return scan<3>("pgdvs_jpeg_scan", coef, B, nby, nbx, restart_mcus, out, out_stride, nbytes, workspace, workspace_bytes, as_stream(stream));
}

PGDVS_API int pgdvs_jpeg_coefficients_420(const float *img_planar, int B, int H, int W, const uint16_t *qtab_luma,
                                          const uint16_t *qtab_chroma, int16_t *coef, pgdvs_stream_t stream) {
  return coefficients("pgdvs_jpeg_coefficients_420", 6, img_planar, B, H, W, qtab_luma, qtab_chroma, coef, as_stream(stream));
}

PGDVS_API int64_t pgdvs_jpeg_scan_420_workspace_bytes(int B, int nmy, int nmx, int restart_mcus) {
  return scan_workspace_bytes("pgdvs_jpeg_scan_420_workspace_bytes", 6, B, nmy, nmx, restart_mcus);
}

PGDVS_API int pgdvs_jpeg_scan_420(const int16_t *coef, int B, int nmy, int nmx, int restart_mcus, uint8_t *out, int64_t out_stride,
                                  int32_t *nbytes, void *workspace, int64_t workspace_bytes, pgdvs_stream_t stream) {
  return scan<6>("pgdvs_jpeg_scan_420", coef, B, nmy, nmx, restart_mcus, out, out_stride, nbytes, workspace, workspace_bytes, as_stream(stream));
}
