// Step 5 kernels: exact all-pairs k-NN on clipped z-score hundredths.
//
// Replaces sklearn NearestNeighbors(brute, euclidean) as called by
// grid/utils/find_neighbors.py:207-213.  Clipped z values are integers
// |q| <= qmax <= 256 (hundredths), exactly representable in bf16, so the Gram
// matrix G = Z Z^T is computed EXACTLY on the bf16 MFMA pipe:
//   * fp32 MFMA accumulators hold partial sums of a few K-steps of 64
//     products, kept below 2^24 so every fp32 partial is an exact integer;
//   * they are then flushed into int32 accumulators (exact while a K-slice
//     stays below 2^31 / qmax^2 products);
//   * each workgroup owns one 256x128 output tile (k_gram8, persistent; the
//     128x128 k_gram_dma covers np % 256 != 0) of one K-slice and adds its int32
//     tile into the int64 Gram with integer atomics (order-free, exact).
// The upper tiles are mirrored into the lower triangle (k_mirror) so a row of
// G is contiguous for the row top-k and the multi-GPU reduce-scatter.
// d2(i,j) = G_ii + G_jj - 2 G_ij is then exact, and neighbours are ordered by
// (d2, j).  That equals sklearn's order wherever exact distances differ.
#include <vector>

#include "common.hpp"

#include <algorithm>
#include <cstdlib>

namespace {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(16))) float f32x16;

constexpr int BM = 128;
constexpr int BK = 64;              // bf16 elements per K-step (128 B per row)
constexpr int NT = 256;             // threads per workgroup (4 waves, 2x2)
constexpr int TILE_BYTES = BM * BK * 2;   // 16 KiB

// LDS image: [row][8 chunks of 16 B], chunk XOR-swizzled by (row>>1)&7 so the
// ds_read_b128 lane groups of the 32x32x16 fragment reads are conflict-free.
__device__ __forceinline__ int lds_off(int row, int chunk) {
  return row * 128 + ((chunk ^ ((row >> 1) & 7)) << 4);
}

__device__ __forceinline__ bf16x8 as_bf16x8(uint4 v) {
  return __builtin_bit_cast(bf16x8, v);
}

// k_gram_dma: LDS-DMA staging (global_load_lds_dwordx4, 1 KiB per wave
// instruction written lane-linearly).  The XOR swizzle moves to the per-lane
// SOURCE address: lane L of an 8-row piece loads chunk (L&7)^((row>>1)&7) of
// row r0+L/8, so the lane-linear LDS image equals lds_off() layout.
typedef __attribute__((address_space(1))) const void *gptr_t;
typedef __attribute__((address_space(3))) void *lptr_t;

__global__ __launch_bounds__(NT, 2) void k_gram_dma(const uint16_t *__restrict__ z, int64_t ld, int nt,
                                                    int ntiles, int64_t nsteps, int sps, int fs,
                                                    int64_t np_, unsigned long long *__restrict__ gram) {
  __shared__ __attribute__((aligned(16))) char smem[2 * 2 * TILE_BYTES];
  const int nwg = gridDim.x;
  const int bid = blockIdx.x;
  const int xcd = bid & 7, loc = bid >> 3;
  const int q8 = nwg >> 3, r8 = nwg & 7;
  const int wid = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + loc;
  const int slice = wid / ntiles;
  int t = wid - slice * ntiles;
  int ti = 0;                                    // upper-triangle tile t -> (ti, tj), row-major
  while (t >= nt - ti) { t -= nt - ti; ti++; }
  const int tj = ti + t;
  const int64_t s0 = (int64_t)slice * sps;
  int64_t s1 = s0 + sps;
  if (s1 > nsteps) s1 = nsteps;

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;

  // this lane's source rows/chunks for its wave's 4 pieces (rows wave*32 + u*8 + lane/8)
  const int prow = wave * 32 + (lane >> 3);          // + u*8
  const uint16_t *za = z + (int64_t)ti * BM * ld;
  const uint16_t *zb = z + (int64_t)tj * BM * ld;
  int64_t srcoff[4];
#pragma unroll
  for (int u = 0; u < 4; u++) {
    const int row = prow + u * 8;
    const int c = (lane & 7) ^ ((row >> 1) & 7);
    srcoff[u] = (int64_t)row * ld + c * 8;
  }

  f32x16 acc[2][2];
  int32_t iacc[2][2][16];
#pragma unroll
  for (int a = 0; a < 2; a++)
#pragma unroll
    for (int b = 0; b < 2; b++)
#pragma unroll
      for (int r = 0; r < 16; r++) { acc[a][b][r] = 0.0f; iacc[a][b][r] = 0; }

#define GRAM_DMA(step, b)                                                                       \
  do {                                                                                         \
    char *A_ = smem + (b) * 2 * TILE_BYTES;                                                     \
    char *B_ = A_ + TILE_BYTES;                                                                 \
    const int64_t k_ = (step) * BK;                                                             \
    _Pragma("unroll") for (int u = 0; u < 4; u++) {                                             \
      __builtin_amdgcn_global_load_lds((gptr_t)(za + srcoff[u] + k_),                           \
                                       (lptr_t)(A_ + (wave * 32 + u * 8) * 128), 16, 0, 0);      \
      __builtin_amdgcn_global_load_lds((gptr_t)(zb + srcoff[u] + k_),                           \
                                       (lptr_t)(B_ + (wave * 32 + u * 8) * 128), 16, 0, 0);      \
    }                                                                                           \
  } while (0)

  // one K-step of MFMAs on LDS buffer `b_`; ZERO_ starts a new fp32 chunk by
  // feeding a zero accumulator to the first MFMA (no separate clearing pass)
#define GRAM_COMPUTE(b_, ZERO_)                                                                \
  do {                                                                                        \
    const char *A = smem + (b_) * 2 * TILE_BYTES;                                              \
    const char *B = A + TILE_BYTES;                                                            \
    _Pragma("unroll") for (int s = 0; s < 4; s++) {                                            \
      const int ch = 2 * s + (lane >> 5);                                                      \
      bf16x8 fa[2], fb[2];                                                                     \
      _Pragma("unroll") for (int m = 0; m < 2; m++) {                                          \
        fa[m] = as_bf16x8(*reinterpret_cast<const uint4 *>(A + lds_off(wr * 64 + m * 32 + (lane & 31), ch))); \
        fb[m] = as_bf16x8(*reinterpret_cast<const uint4 *>(B + lds_off(wc * 64 + m * 32 + (lane & 31), ch))); \
      }                                                                                        \
      _Pragma("unroll") for (int m = 0; m < 2; m++)                                            \
        _Pragma("unroll") for (int nn = 0; nn < 2; nn++)                                       \
          acc[m][nn] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[m], fb[nn],                  \
                                                               (ZERO_ && s == 0) ? zero16 : acc[m][nn], 0, 0, 0); \
    }                                                                                          \
  } while (0)

  const f32x16 zero16 = {};
  if (s0 < s1) GRAM_DMA(s0, 0);
  __syncthreads();
  int buf = 0;
  for (int64_t cs = s0; cs < s1; cs += fs) {
    const int64_t ce = (cs + fs < s1) ? cs + fs : s1;
    // first step of the chunk: fresh fp32 partials
    if (cs + 1 < s1) GRAM_DMA(cs + 1, buf ^ 1);
    GRAM_COMPUTE(buf, true);
    __syncthreads();
    buf ^= 1;
    for (int64_t st = cs + 1; st < ce; st++) {
      if (st + 1 < s1) GRAM_DMA(st + 1, buf ^ 1);
      GRAM_COMPUTE(buf, false);
      __syncthreads();     // drains this wave's DMA (vmcnt) and orders all reads of buf
      buf ^= 1;
    }
    // flush: exact fp32 partials (< 2^24) into int32
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
      for (int b = 0; b < 2; b++)
#pragma unroll
        for (int r = 0; r < 16; r++) iacc[a][b][r] += (int32_t)acc[a][b][r];
  }
#undef GRAM_COMPUTE
#undef GRAM_DMA
#pragma unroll
  for (int a = 0; a < 2; a++)
#pragma unroll
    for (int b = 0; b < 2; b++)
#pragma unroll
      for (int r = 0; r < 16; r++) {
        int row = ti * BM + wr * 64 + a * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        int col = tj * BM + wc * 64 + b * 32 + (lane & 31);
        int32_t v = iacc[a][b][r];
        if (v != 0) atomicAdd(gram + (int64_t)row * np_ + col, (unsigned long long)(long long)v);
      }
}

constexpr int BM3 = 256, BN3 = 128;
constexpr bool GRAM_WIDE = false;   // default for GRID_GRAM_WIDE (16x16 layout: flush in 512-B row segments)
constexpr int SLOT3 = (BM3 + BN3) * BK * 2;     // 48 KiB
constexpr int QSA = BM3 * BK * 2, QSB = BN3 * BK * 2;   // quad-row image: A / B slot bytes

// Work map of k_gram8: 256x128 tiles (I, j >= 2I) in 4x8 super-blocks, so the
// workgroups of one XCD round share 4 A and 8 B panels in its L2
// (launch_gram8 enumerates the tiles in that order).
constexpr int GI6 = 4, GJ6 = 8;

// Drain iacc into the int64 Gram (order-free integer atomics) and clear it.
template <int MB>
__device__ __forceinline__ void g6_atomics(int32_t (&iacc)[MB][2][16], int I, int tj, int64_t np_,
                                           unsigned long long *__restrict__ gram) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wr = wave >> 1, wc = wave & 1;
#pragma unroll
  for (int a = 0; a < MB; a++)
#pragma unroll
    for (int b = 0; b < 2; b++)
#pragma unroll
      for (int r = 0; r < 16; r++) {
        int row = I * BM3 + wr * (32 * MB) + a * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        int col = tj * BN3 + wc * 64 + b * 32 + (lane & 31);
        int32_t v = iacc[a][b][r];
        if (v != 0) atomicAdd(gram + (int64_t)row * np_ + col, (unsigned long long)(long long)v);
        iacc[a][b][r] = 0;
      }
}

// Plain-store flush (k_gram8 partial mode): the unit's int32 tile, row-major
// [256][128] in its own scratch slot (one 128-B row segment per half-wave
// store), summed per tile by k_gram_part_reduce after the launch.  A
// workgroup's 128 KiB of plain stores drain in a few us where its 256 KiB of
// int64 atomics took tens (atomics run at ~1.3 TB/s chip-wide).
template <int MB>
__device__ __forceinline__ void g8_store_part(int32_t (&iacc)[MB][2][16], int32_t *__restrict__ slot) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wr = wave >> 1, wc = wave & 1;
#pragma unroll
  for (int a = 0; a < MB; a++)
#pragma unroll
    for (int b = 0; b < 2; b++)
#pragma unroll
      for (int r = 0; r < 16; r++) {
        const int row = wr * (32 * MB) + a * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        const int col = wc * 64 + b * 32 + (lane & 31);
        slot[row * BN3 + col] = iacc[a][b][r];
        iacc[a][b][r] = 0;
      }
}

// Slot offsets of the XCDs' unit ranges (partial mode), passed by value.
struct GramXoff {
  int64_t x[8];
};

// gram tile t += the sum (int64, exact in any order) of its units' slots; the
// units of tile t follow k_gram8's unit -> (group, chunk, tile) map: group
// g = t / per is run by the XCDs x = (g % gx) * kx + kr (kr < kx), unit
// u = (g / gx) * per * kc + c * gsz + t % per for chunk c (empty K ranges
// hold no slot).  One thread per tile element.
__global__ __launch_bounds__(256) void k_gram_part_reduce(const int32_t *__restrict__ part, GramXoff xo, int per,
                                                          int kc, int kx, int64_t nsteps, int ntiles,
                                                          const int32_t *__restrict__ tiles, int64_t np_,
                                                          int64_t *__restrict__ gram) {
  const int e = blockIdx.x * 256 + threadIdx.x;            // element of the 256 x 128 tile
  const int t = blockIdx.y;
  const int gx = 8 / kx, g = t / per, tl = t % per;
  const int gsz = min(per, ntiles - g * per);
  int64_t sum = 0;
  for (int kr = 0; kr < kx; kr++) {
    const int x = (g % gx) * kx + kr;
    const int64_t xs0 = nsteps * kr / kx, xlen = nsteps * (kr + 1) / kx - xs0;
    for (int c = 0; c < kc; c++) {
      if (xlen * c / kc == xlen * (c + 1) / kc) continue;
      const int64_t u = (int64_t)(g / gx) * per * kc + (int64_t)c * gsz + tl;
      sum += part[(xo.x[x] + u) * (BM3 * BN3) + e];
    }
  }
  const int32_t tv = tiles[t];
  const int64_t row = (int64_t)(tv >> 16) * BM3 + e / BN3, col = (int64_t)(tv & 0xFFFF) * BN3 + e % BN3;
  gram[row * np_ + col] += sum;
}

template <int MB>
__device__ __forceinline__ void g6_zero(f32x16 (&acc)[MB][2], int32_t (&iacc)[MB][2][16]) {
#pragma unroll
  for (int a = 0; a < MB; a++)
#pragma unroll
    for (int b = 0; b < 2; b++)
#pragma unroll
      for (int r = 0; r < 16; r++) { acc[a][b][r] = 0.0f; iacc[a][b][r] = 0; }
}

// Default Gram kernel (k_gram8): persistent, one 512-thread workgroup per CU,
// XCD x = blockIdx % 8 (placement is a performance assumption only; results
// never depend on it).  XCD x owns K-steps [x*S/8, (x+1)*S/8) split into kc
// chunks; its workgroups walk the units (tile group g, chunk c, tile) in
// ROUNDS of `per`, so in any round they read the same K range of the same few
// A/B panels and the XCD's L2 serves each panel byte to up to 8 workgroups.
// A bounded spin on a per-XCD round counter keeps them in step (never a
// correctness barrier).  Every unit is at most sps_max K-steps (int32-exact)
// and drains its iacc with int64 atomics.
//
// The K loop does no address arithmetic and fits 256 registers without
// spills (a spill reload's vmcnt(0) would drain the LDS-DMA ring):
//   * LDS: a ring of 3 slots of 48 KiB (a K-step of 256 A and 128 B rows); one
//     VGPR per fragment base, the slot and sub-step as immediate offsets.  The
//     images (conflict-free for ds_read_b128) are described at g8_run (quad-row,
//     row-major panel), g8h_run and g8q_run (half-split, K-blocked panel).
//   * DMA: buffer_load_dwordx4 ... lds in whole 64-B row pieces.  Panel base in
//     the descriptor (SGPRs), row offsets in VGPRs, the K offset in soffset.
//   * BL: the panel is K-blocked, [kpad / 32][row][32] (the layout zquant writes
//     for the fused chain): a K-half of a 256-row panel is one contiguous
//     16 KiB run instead of 256 rows 2*ld bytes apart (-9 % time: fewer pages
//     and DRAM rows per step).
//   * fp32 chunks: a 6-step group (24 sub-steps) walks the 3 ring slots twice,
//     so slots are compile-time; block b = 2m + nn restarts its fp32 chunk at
//     sub-steps 6b (FL = 1: 384-product chunks, exact while 384 qmax^2 <= 2^24,
//     qmax <= 209) or 3b and 12 + 3b (FL = 2: 192 products, qmax <= 256).
template <int OFF>
__device__ __forceinline__ uint4 lds_rd(uint32_t addr) {
  uint4 v;
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "i"(OFF));
  return v;
}

// Row-major panel, quad-row image: a lane quad of every LDS-DMA piece reads 64
// contiguous bytes of ONE panel row (the texture path then moves a piece at
// twice the rate of pieces whose lane pairs read 32 B: 146 vs 75 GB/s per CU
// from L2, tools/micro/dmapat.hip).  Piece (8-row block b) = [half p (2)][row r (8)][64 B],
// the 16-B chunk j of a half stored at j ^ (b & 3); A slots at 0/32/64 KiB,
// B slots at 96/112/128 KiB.  Fragment of sub-step s = chunk 2s + h of row R:
// base(s & 1) + 512 (s >> 1) (+ slot offset), where the odd base is the even one
// ^ 32; each ds_read_b128 lane group sees 4 rows x 4 distinct x = b & 3, i.e.
// 16 distinct 16-B bank slots (conflict-free).
template <int FL>
__device__ __forceinline__ void g8_run(const uint16_t *__restrict__ z, int64_t ld, int I, int tj, int64_t s0,
                                       int64_t s1, char *smem, f32x16 (&acc)[2][2],
                                       int32_t (&iacc)[2][2][16]) {
  constexpr int NF = 4, NDMA = 6;
  constexpr int FCYC = 24 / FL, FSP = FCYC / 4;   // flush cycle and stagger, in sub-steps
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int wr = wv >> 1, wc = wv & 1;
  // DMA sources: this wave's 32 A rows and 16 B rows; base in the descriptor,
  // K offset in soffset.
  const int64_t rs_el = ld;                                                    // row stride (elements)
  const uint16_t *pa0 = z + ((int64_t)I * BM3 + wv * 32) * rs_el;
  const uint16_t *pb0 = z + ((int64_t)tj * BN3 + wv * 16) * rs_el;
  const __amdgpu_buffer_rsrc_t rsa = __builtin_amdgcn_make_buffer_rsrc((void *)pa0, (short)0, -1, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsb = __builtin_amdgcn_make_buffer_rsrc((void *)pb0, (short)0, -1, 0x00020000);
  const uint32_t rb8 = (uint32_t)(16 * rs_el);                                 // bytes per 8 rows
  const int qr = (lane >> 2) & 7, qp = lane >> 5, qj = lane & 3;
  auto vq = [&](int x) { return (uint32_t)((qr * rs_el + (4 * qp + (qj ^ x)) * 8) * 2); };
  const uint32_t vo0 = vq(0), vo1 = vq(1) + rb8, vo2 = vq(2) + 2 * rb8, vo3 = vq(3) + 3 * rb8;
  const int xb = 2 * (wv & 1);                                                 // B blocks 2 wv + t
  const uint32_t vb0 = vq(xb), vb1 = vq(xb + 1) + rb8;
  const uint32_t sbase = (uint32_t)(uintptr_t)smem;
  // fragment bases per (parity of s, fragment): A blocks m = 0, 1; B blocks
  // nn = 0, 1; slot 2 of A separately (offsets stay < 64 KiB)
  uint32_t ad[3][4];
#pragma unroll
  for (int f = 0; f < 4; f++) {
    const int R = f < 2 ? wr * 64 + f * 32 + (lane & 31) : wc * 64 + (f - 2) * 32 + (lane & 31);
    const int rb = R >> 3;
    const uint32_t ev = sbase + (f < 2 ? 0 : 3 * QSA) + rb * 1024 + (R & 7) * 64 + (((lane >> 5) ^ (rb & 3)) << 4);
    ad[0][f] = ev;
    ad[1][f] = ev ^ 32u;
    if (f < 2) {                        // A, slot 2: [2][m] even, [2][2 + m] odd
      ad[2][f] = ev + 2 * QSA;
      ad[2][f + 2] = (ev ^ 32u) + 2 * QSA;
    }
  }
  const f32x16 zero16 = {};
  uint4 fr0[NF], fr1[NF];

#define G8_WAIT_VM(n_) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(n_) : "memory")
#define G8_WAIT_LGKM(n_) asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(n_) : "memory")
#define G8_SB() __builtin_amdgcn_sched_barrier(0)
#define G8_ISSUE(step_, SL)                                                                    \
  do {                                                                                         \
    const uint32_t so_ = (uint32_t)((step_) * (BK * 2));                                       \
    char *A_ = smem + (SL) * QSA + wv * 4096;                                                  \
    char *B_ = smem + 3 * QSA + (SL) * QSB + wv * 2048;                                        \
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsa, (lptr_t)(A_), 16, vo0, so_, 0, 0);           \
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsa, (lptr_t)(A_ + 1024), 16, vo1, so_, 0, 0);    \
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsa, (lptr_t)(A_ + 2048), 16, vo2, so_, 0, 0);    \
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsa, (lptr_t)(A_ + 3072), 16, vo3, so_, 0, 0);    \
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsb, (lptr_t)(B_), 16, vb0, so_, 0, 0);           \
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsb, (lptr_t)(B_ + 1024), 16, vb1, so_, 0, 0);    \
  } while (0)
#define G8_READ(FR, SL, s_)                                                                    \
  do {                                                                                         \
    constexpr int pa_ = (s_) & 1, ia_ = (SL) == 2 ? 2 : pa_, ja_ = (SL) == 2 ? 2 * pa_ : 0;    \
    constexpr int oa_ = ((SL) == 2 ? 0 : (SL) * QSA) + ((s_) >> 1) * 512;                      \
    constexpr int ob_ = (SL) * QSB + ((s_) >> 1) * 512;                                        \
    FR[0] = lds_rd<oa_>(ad[ia_][ja_]);                                                         \
    FR[1] = lds_rd<oa_>(ad[ia_][ja_ + 1]);                                                     \
    FR[2] = lds_rd<ob_>(ad[pa_][2]);                                                           \
    FR[3] = lds_rd<ob_>(ad[pa_][3]);                                                           \
  } while (0)
  // MFMAs of A blocks [m0, m1) at in-group sub-step c_; block b = 2m + nn starts
  // a new fp32 chunk (after flushing the old one) at sub-steps = FSP b (mod FCYC)
#define G8_MFMA(FR, c_, m0, m1, STAG)                                                          \
  do {                                                                                         \
    _Pragma("unroll") for (int m = m0; m < m1; m++)                                            \
      _Pragma("unroll") for (int nn = 0; nn < 2; nn++) {                                       \
        if ((STAG) && ((c_) % FCYC) == FSP * (m * 2 + nn)) {                                   \
          _Pragma("unroll") for (int r = 0; r < 16; r++) iacc[m][nn][r] += (int32_t)acc[m][nn][r]; \
          acc[m][nn] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_bf16x8(FR[m]), as_bf16x8(FR[2 + nn]), \
                                                               zero16, 0, 0, 0);               \
        } else {                                                                               \
          acc[m][nn] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_bf16x8(FR[m]), as_bf16x8(FR[2 + nn]), \
                                                               acc[m][nn], 0, 0, 0);           \
        }                                                                                      \
      }                                                                                        \
  } while (0)
  // K-step st_ in ring slot SL (compile-time), in-group index q_; fr0 holds
  // its sub-step 0 on entry and the next step's sub-step 0 on exit.  The
  // barrier sits inside the last sub-step; the slot it frees receives st_ + 3.
#define G8_STEP(st_, q_, SL, STAG, COND)                                                       \
  do {                                                                                        \
    G8_READ(fr1, SL, 1);                                                                       \
    G8_WAIT_LGKM(NF); G8_SB();                                                                 \
    G8_MFMA(fr0, 4 * (q_) + 0, 0, 2, STAG); G8_SB();                                           \
    G8_READ(fr0, SL, 2);                                                                       \
    G8_WAIT_LGKM(NF); G8_SB();                                                                 \
    G8_MFMA(fr1, 4 * (q_) + 1, 0, 2, STAG); G8_SB();                                           \
    G8_READ(fr1, SL, 3);                                                                       \
    G8_WAIT_LGKM(NF); G8_SB();                                                                 \
    G8_MFMA(fr0, 4 * (q_) + 2, 0, 2, STAG); G8_SB();                                           \
    G8_WAIT_LGKM(0); G8_SB();                                                                  \
    G8_MFMA(fr1, 4 * (q_) + 3, 0, 1, STAG); G8_SB();                                           \
    if (!(COND) || (st_) + 2 < s1) G8_WAIT_VM(NDMA);                                           \
    else G8_WAIT_VM(0);                                                                        \
    __builtin_amdgcn_s_barrier(); G8_SB();                                                     \
    if (!(COND) || (st_) + 3 < s1) G8_ISSUE((st_) + 3, SL);                                    \
    if (!(COND) || (st_) + 1 < s1) G8_READ(fr0, ((SL) + 1) % 3, 0);                            \
    G8_SB();                                                                                   \
    G8_MFMA(fr1, 4 * (q_) + 3, 1, 2, STAG); G8_SB();                                           \
  } while (0)
#define G8_FLUSH()                                                                             \
  do {                                                                                        \
    _Pragma("unroll") for (int a = 0; a < 2; a++)                                              \
      _Pragma("unroll") for (int b = 0; b < 2; b++)                                            \
        _Pragma("unroll") for (int r = 0; r < 16; r++) {                                       \
          iacc[a][b][r] += (int32_t)acc[a][b][r];                                              \
          acc[a][b][r] = 0.0f;                                                                 \
        }                                                                                      \
  } while (0)

  if (s0 >= s1) return;
  G8_ISSUE(s0, 0);
  if (s0 + 1 < s1) G8_ISSUE(s0 + 1, 1);
  if (s0 + 2 < s1) G8_ISSUE(s0 + 2, 2);
  if (s0 + 2 < s1) G8_WAIT_VM(2 * NDMA);
  else if (s0 + 1 < s1) G8_WAIT_VM(NDMA);
  else G8_WAIT_VM(0);
  __builtin_amdgcn_s_barrier();
  G8_SB();
  G8_READ(fr0, 0, 0);
  int64_t st = s0;
  const int64_t sfull = s0 + ((s1 - s0) / 6) * 6;
  // steady state: every step's DMA lead (st + 3) exists
  for (; st < sfull && st + 8 < s1; st += 6) {
    G8_STEP(st, 0, 0, 1, 0);
    G8_STEP(st + 1, 1, 1, 1, 0);
    G8_STEP(st + 2, 2, 2, 1, 0);
    G8_STEP(st + 3, 3, 0, 1, 0);
    G8_STEP(st + 4, 4, 1, 1, 0);
    G8_STEP(st + 5, 5, 2, 1, 0);
  }
  for (; st < sfull; st += 6) {
    G8_STEP(st, 0, 0, 1, 1);
    G8_STEP(st + 1, 1, 1, 1, 1);
    G8_STEP(st + 2, 2, 2, 1, 1);
    G8_STEP(st + 3, 3, 0, 1, 1);
    G8_STEP(st + 4, 4, 1, 1, 1);
    G8_STEP(st + 5, 5, 2, 1, 1);
  }
  G8_FLUSH();
  // tail (< 6 steps): slot (st - s0) % 3 known at run time; one fp32 chunk
  // for FL = 1 (<= 320 products), flushed every 3 steps for FL = 2
  for (int t = 0; st < s1; st++, t++) {
    const int sl = (int)((st - s0) % 3);
    if (sl == 0) G8_STEP(st, 0, 0, 0, 1);
    else if (sl == 1) G8_STEP(st, 0, 1, 0, 1);
    else G8_STEP(st, 0, 2, 0, 1);
    if (FL == 2 && t == 2) G8_FLUSH();
  }
  G8_FLUSH();
#undef G8_WAIT_VM
#undef G8_WAIT_LGKM
#undef G8_SB
#undef G8_ISSUE
#undef G8_READ
#undef G8_MFMA
#undef G8_STEP
#undef G8_FLUSH
}

// LAY 3 (K-blocked panel, half-split image): every ring slot holds a K-step as
// two halves (K chunks 0-3 | 4-7, 64 B of each panel row), region [half p][row][64 B]
// with the 16-B chunk j of row R stored at j ^ ((R >> 2) & 3).  A DMA piece is
// 16 rows x 64 B (lane quad = 64 contiguous bytes of one row; ONE voffset VGPR,
// the piece's rows in soffset, its K-half in the descriptor base: a K-block
// stride of ld / 2 elements exceeds 32-bit offsets).  Sub-steps 0-1 read half 0 and 2-3
// half 1, so each half of slot st is refilled with step st + 3 as soon as
// every wave has read it: two barriers per step, each followed by 3 pieces
// per wave (the texture path's work spread over the step instead of one
// 6-piece burst behind a single barrier), and 2.5 steps of DMA lead.
// Fragment bases: even / odd sub-steps (odd = even ^ 32), half offsets and
// slots as immediates (A slot 2 has its own bases: offsets stay < 64 KiB).
// The panel is K-blocked by 32 columns, [K-half][row][32], so a 16-row half
// piece is 1 KiB contiguous (whole 128-B lines).
// FL = 1 is kept only for the GRID_ISA_PROBE pair (tools/isa_barriers.py --probe); the product runs FL = 2 here.
template <int FL>
__device__ __forceinline__ void g8h_run(const uint16_t *__restrict__ z, int64_t ld, int I, int tj, int64_t s0,
                                        int64_t s1, char *smem, f32x16 (&acc)[2][2],
                                        int32_t (&iacc)[2][2][16]) {
  constexpr int NF = 4;
  constexpr int FCYC = 24 / FL, FSP = FCYC / 4;
  constexpr int HA = QSA / 2, HB = QSB / 2;             // half regions of a slot (A, B)
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int wr = wv >> 1, wc = wv & 1;
  constexpr int64_t rs_el = BK / 2;                     // 64-B rows
  const uint16_t *pa0 = z + ((int64_t)I * BM3 + wv * 32) * rs_el;
  const uint16_t *pb0 = z + ((int64_t)tj * BN3 + wv * 16) * rs_el;
  const uint32_t vq = (uint32_t)(((lane >> 2) * rs_el + ((lane & 3) ^ ((lane >> 4) & 3)) * 8) * 2);
  const uint32_t r16 = (uint32_t)(32 * rs_el);         // bytes per 16 rows
  const uint32_t sbase = (uint32_t)(uintptr_t)smem;
  uint32_t ad[3][4];
#pragma unroll
  for (int f = 0; f < 4; f++) {
    const int R = f < 2 ? wr * 64 + f * 32 + (lane & 31) : wc * 64 + (f - 2) * 32 + (lane & 31);
    const uint32_t ev = sbase + (f < 2 ? 0 : 3 * QSA) + R * 64 + ((((lane >> 5) ^ (R >> 2)) & 3) << 4);
    ad[0][f] = ev;
    ad[1][f] = ev ^ 32u;
    if (f < 2) {                      // A, slot 2: [2][m] even, [2][2 + m] odd
      ad[2][f] = ev + 2 * QSA;
      ad[2][f + 2] = (ev ^ 32u) + 2 * QSA;
    }
  }
  const f32x16 zero16 = {};
  uint4 fr0[NF], fr1[NF];

#define H8_WAIT_VM(n_) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(n_) : "memory")
#define H8_WAIT_LGKM(n_) asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(n_) : "memory")
#define H8_SB() __builtin_amdgcn_sched_barrier(0)
  // half P of K-step step_ into ring slot SL: A rows wv*32 + {0..15, 16..31}, B rows wv*16 + 0..15
#define H8_ISSUE(step_, P, SL)                                                                 \
  do {                                                                                         \
    const int64_t ko_ = (2 * (int64_t)(step_) + (P)) * (ld >> 1);                              \
    const __amdgpu_buffer_rsrc_t rsa = __builtin_amdgcn_make_buffer_rsrc(                      \
        (void *)(pa0 + ko_), (short)0, -1, 0x00020000);                                        \
    const __amdgpu_buffer_rsrc_t rsb = __builtin_amdgcn_make_buffer_rsrc(                      \
        (void *)(pb0 + ko_), (short)0, -1, 0x00020000);                                        \
    char *A_ = smem + (SL) * QSA + (P) * HA + wv * 2048;                                       \
    char *B_ = smem + 3 * QSA + (SL) * QSB + (P) * HB + wv * 1024;                             \
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsa, (lptr_t)(A_), 16, vq, 0, 0, 0);              \
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsa, (lptr_t)(A_ + 1024), 16, vq, r16, 0, 0);     \
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsb, (lptr_t)(B_), 16, vq, 0, 0, 0);              \
  } while (0)
#define H8_READ(FR, SL, s_)                                                                    \
  do {                                                                                         \
    constexpr int pa_ = (s_) & 1, ia_ = (SL) == 2 ? 2 : pa_, ja_ = (SL) == 2 ? 2 * pa_ : 0;    \
    constexpr int oa_ = ((SL) == 2 ? 0 : (SL) * QSA) + ((s_) >> 1) * HA;                       \
    constexpr int ob_ = (SL) * QSB + ((s_) >> 1) * HB;                                         \
    FR[0] = lds_rd<oa_>(ad[ia_][ja_]);                                                         \
    FR[1] = lds_rd<oa_>(ad[ia_][ja_ + 1]);                                                     \
    FR[2] = lds_rd<ob_>(ad[pa_][2]);                                                           \
    FR[3] = lds_rd<ob_>(ad[pa_][3]);                                                           \
  } while (0)
#define H8_MFMA(FR, c_, m0, m1, STAG)                                                          \
  do {                                                                                         \
    _Pragma("unroll") for (int m = m0; m < m1; m++)                                            \
      _Pragma("unroll") for (int nn = 0; nn < 2; nn++) {                                       \
        if ((STAG) && ((c_) % FCYC) == FSP * (m * 2 + nn)) {                                   \
          _Pragma("unroll") for (int r = 0; r < 16; r++) iacc[m][nn][r] += (int32_t)acc[m][nn][r]; \
          acc[m][nn] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_bf16x8(FR[m]), as_bf16x8(FR[2 + nn]), \
                                                               zero16, 0, 0, 0);               \
        } else {                                                                               \
          acc[m][nn] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_bf16x8(FR[m]), as_bf16x8(FR[2 + nn]), \
                                                               acc[m][nn], 0, 0, 0);           \
        }                                                                                      \
      }                                                                                        \
  } while (0)
  // vmcnt before barrier 1 of step st: the wave's pieces of (st, half 1) have
  // landed; younger: (st+1, *), (st+2, *) -- 3 pieces per half
#define H8_VM1(st_, COND)                                                                      \
  do {                                                                                        \
    if (!(COND) || (st_) + 2 < s1) H8_WAIT_VM(12);                                             \
    else if ((st_) + 1 < s1) H8_WAIT_VM(6);                                                    \
    else H8_WAIT_VM(0);                                                                        \
  } while (0)
  // before barrier 2: (st+1, half 0) landed; younger: (st+1, 1), (st+2, *), (st+3, 0)
#define H8_VM2(st_, COND)                                                                      \
  do {                                                                                        \
    if (!(COND) || (st_) + 3 < s1) H8_WAIT_VM(12);                                             \
    else if ((st_) + 2 < s1) H8_WAIT_VM(9);                                                    \
    else if ((st_) + 1 < s1) H8_WAIT_VM(3);                                                    \
    else H8_WAIT_VM(0);                                                                        \
  } while (0)
  // K-step st_ in ring slot SL (compile-time), in-group index q_; fr0 holds
  // its sub-step 0 on entry and the next step's sub-step 0 on exit.
#define H8_STEP(st_, q_, SL, STAG, COND)                                                       \
  do {                                                                                        \
    H8_READ(fr1, SL, 1);                                                                       \
    H8_WAIT_LGKM(NF); H8_SB();                                                                 \
    H8_MFMA(fr0, 4 * (q_) + 0, 0, 2, STAG); H8_SB();                                           \
    H8_WAIT_LGKM(0); H8_VM1(st_, COND);                                                        \
    __builtin_amdgcn_s_barrier(); H8_SB();                                                     \
    if (!(COND) || (st_) + 3 < s1) H8_ISSUE((st_) + 3, 0, SL);                                 \
    H8_READ(fr0, SL, 2);                                                                       \
    H8_SB();                                                                                   \
    H8_MFMA(fr1, 4 * (q_) + 1, 0, 2, STAG); H8_SB();                                           \
    H8_READ(fr1, SL, 3);                                                                       \
    H8_WAIT_LGKM(NF); H8_SB();                                                                 \
    H8_MFMA(fr0, 4 * (q_) + 2, 0, 2, STAG); H8_SB();                                           \
    H8_WAIT_LGKM(0); H8_SB();                                                                  \
    H8_MFMA(fr1, 4 * (q_) + 3, 0, 1, STAG); H8_SB();                                           \
    H8_VM2(st_, COND);                                                                         \
    __builtin_amdgcn_s_barrier(); H8_SB();                                                     \
    if (!(COND) || (st_) + 3 < s1) H8_ISSUE((st_) + 3, 1, SL);                                 \
    if (!(COND) || (st_) + 1 < s1) H8_READ(fr0, ((SL) + 1) % 3, 0);                            \
    H8_SB();                                                                                   \
    H8_MFMA(fr1, 4 * (q_) + 3, 1, 2, STAG); H8_SB();                                           \
  } while (0)
#define H8_FLUSH()                                                                             \
  do {                                                                                        \
    _Pragma("unroll") for (int a = 0; a < 2; a++)                                              \
      _Pragma("unroll") for (int b = 0; b < 2; b++)                                            \
        _Pragma("unroll") for (int r = 0; r < 16; r++) {                                       \
          iacc[a][b][r] += (int32_t)acc[a][b][r];                                              \
          acc[a][b][r] = 0.0f;                                                                 \
        }                                                                                      \
  } while (0)

  if (s0 >= s1) return;
  H8_ISSUE(s0, 0, 0);
  H8_ISSUE(s0, 1, 0);
  if (s0 + 1 < s1) { H8_ISSUE(s0 + 1, 0, 1); H8_ISSUE(s0 + 1, 1, 1); }
  if (s0 + 2 < s1) { H8_ISSUE(s0 + 2, 0, 2); H8_ISSUE(s0 + 2, 1, 2); }
  // (s0, half 0) landed; younger: (s0, 1) and the two next steps
  if (s0 + 2 < s1) H8_WAIT_VM(15);
  else if (s0 + 1 < s1) H8_WAIT_VM(9);
  else H8_WAIT_VM(3);
  __builtin_amdgcn_s_barrier();
  H8_SB();
  H8_READ(fr0, 0, 0);
  int64_t st = s0;
  const int64_t sfull = s0 + ((s1 - s0) / 6) * 6;
  for (; st < sfull && st + 8 < s1; st += 6) {
    H8_STEP(st, 0, 0, 1, 0);
    H8_STEP(st + 1, 1, 1, 1, 0);
    H8_STEP(st + 2, 2, 2, 1, 0);
    H8_STEP(st + 3, 3, 0, 1, 0);
    H8_STEP(st + 4, 4, 1, 1, 0);
    H8_STEP(st + 5, 5, 2, 1, 0);
  }
  for (; st < sfull; st += 6) {
    H8_STEP(st, 0, 0, 1, 1);
    H8_STEP(st + 1, 1, 1, 1, 1);
    H8_STEP(st + 2, 2, 2, 1, 1);
    H8_STEP(st + 3, 3, 0, 1, 1);
    H8_STEP(st + 4, 4, 1, 1, 1);
    H8_STEP(st + 5, 5, 2, 1, 1);
  }
  H8_FLUSH();
  for (int t = 0; st < s1; st++, t++) {
    const int sl = (int)((st - s0) % 3);
    if (sl == 0) H8_STEP(st, 0, 0, 0, 1);
    else if (sl == 1) H8_STEP(st, 0, 1, 0, 1);
    else H8_STEP(st, 0, 2, 0, 1);
    if (FL == 2 && t == 2) H8_FLUSH();
  }
  H8_FLUSH();
#undef H8_WAIT_VM
#undef H8_WAIT_LGKM
#undef H8_SB
#undef H8_ISSUE
#undef H8_READ
#undef H8_MFMA
#undef H8_VM1
#undef H8_VM2
#undef H8_STEP
#undef H8_FLUSH
}

// LAY 4: the half-split ring of LAY 3 (K32 panel, same DMA pieces, same
// barriers and vmcnt counts) feeding v_mfma_f32_16x16x32_bf16 instead of
// 32x32x16.  The two shapes take the same cycles per flop, but on random data
// the chip holds a higher clock under the 16x16 loop (MI355X guide, "DVFS
// give-back" item 7: ~1.12-1.15x FLOP/s with LDS-fed operands).  One 16x16x32
// fragment is 16 rows x one whole K-half (64 B per row), so a half is 4 A + 4 B
// fragments (one fragment set per half, double-buffered across halves) and 16
// MFMAs per wave; accumulators f32x4 [4][4] (64 VGPRs, as before).  Image: the
// 16-B chunk j of row R stored at j ^ g((R >> 2) & 3), g = {0, 2, 3, 1}: every
// 16-lane group of a fragment read (rows R & 15 = lane & 15, chunk lane >> 4)
// then hits 16 distinct 16-B bank slots.  Flush stagger: block b = 4m + nn
// restarts its fp32 chunk at half-step (b * FCYC) / 16 of every FCYC-half
// cycle (FCYC = 12 half-steps = 384 products for FL = 1, 6 for FL = 2).
__device__ __forceinline__ int64_t uniform64(int64_t v) {
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v);
  const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)((uint64_t)v >> 32));
  return (int64_t)(((uint64_t)hi << 32) | lo);
}

__device__ __forceinline__ int g8q_swz(int rb) { return (0x78 >> (2 * (rb & 3))) & 3; }

typedef __attribute__((ext_vector_type(4))) float f32x4;

template <int FL>
__device__ __forceinline__ void g8q_run(const uint16_t *__restrict__ z, int64_t ld, int I, int tj, int64_t s0,
                                        int64_t s1, char *smem, f32x4 (&acc)[4][4], int32_t (&iacc)[4][4][4]) {
  constexpr int FCYC = 12 / FL;                          // fp32 chunk, in half-steps
  constexpr int HA = QSA / 2, HB = QSB / 2;
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int wr = wv >> 1, wc = wv & 1;
  constexpr int64_t rs_el = BK / 2;                      // K32 panel: 64-B rows
  const uint16_t *pa0 = z + ((int64_t)I * BM3 + wv * 32) * rs_el;
  const uint16_t *pb0 = z + ((int64_t)tj * BN3 + wv * 16) * rs_el;
  const uint32_t vq = (uint32_t)(((lane >> 2) * rs_el + ((lane & 3) ^ g8q_swz(lane >> 4)) * 8) * 2);
  const uint32_t r16 = (uint32_t)(32 * rs_el);           // bytes per 16 rows
  const uint32_t sbase = (uint32_t)(uintptr_t)smem;
  const uint32_t la = (uint32_t)((lane & 15) * 64 + (((lane >> 4) ^ g8q_swz(lane >> 2)) << 4));
  const uint32_t ba = sbase + wr * 64 * 64 + la;         // A slots 0, 1 (immediate slot offsets)
  const uint32_t ba2 = ba + 2 * QSA;                     // A slot 2 (offsets stay < 64 KiB)
  const uint32_t bb = sbase + 3 * QSA + wc * 64 * 64 + la;
  const f32x4 zero4 = {};
  uint4 F0[8], F1[8];

#define Q8_WAIT_VM(n_) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(n_) : "memory")
#define Q8_WAIT_LGKM(n_) asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(n_) : "memory")
#define Q8_SB() __builtin_amdgcn_sched_barrier(0)
#define Q8_ISSUE(step_, P, SL)                                                                 \
  do {                                                                                         \
    const int64_t ko_ = (2 * (int64_t)(step_) + (P)) * (ld >> 1);                              \
    const __amdgpu_buffer_rsrc_t rsa = __builtin_amdgcn_make_buffer_rsrc(                      \
        (void *)(pa0 + ko_), (short)0, -1, 0x00020000);                                        \
    const __amdgpu_buffer_rsrc_t rsb = __builtin_amdgcn_make_buffer_rsrc(                      \
        (void *)(pb0 + ko_), (short)0, -1, 0x00020000);                                        \
    char *A_ = smem + (SL) * QSA + (P) * HA + wv * 2048;                                       \
    char *B_ = smem + 3 * QSA + (SL) * QSB + (P) * HB + wv * 1024;                             \
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsa, (lptr_t)(A_), 16, vq, 0, 0, 0);              \
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsa, (lptr_t)(A_ + 1024), 16, vq, r16, 0, 0);     \
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsb, (lptr_t)(B_), 16, vq, 0, 0, 0);              \
  } while (0)
  // the 8 fragments (A m = 0..3, B nn = 0..3) of half P of ring slot SL
#define Q8_READ(FR, SL, P)                                                                     \
  do {                                                                                         \
    constexpr int oa_ = ((SL) == 2 ? 0 : (SL) * QSA) + (P) * HA;                               \
    constexpr int ob_ = (SL) * QSB + (P) * HB;                                                 \
    const uint32_t a_ = (SL) == 2 ? ba2 : ba;                                                  \
    FR[0] = lds_rd<oa_>(a_); FR[1] = lds_rd<oa_ + 1024>(a_);                                   \
    FR[2] = lds_rd<oa_ + 2048>(a_); FR[3] = lds_rd<oa_ + 3072>(a_);                            \
    FR[4] = lds_rd<ob_>(bb); FR[5] = lds_rd<ob_ + 1024>(bb);                                   \
    FR[6] = lds_rd<ob_ + 2048>(bb); FR[7] = lds_rd<ob_ + 3072>(bb);                            \
  } while (0)
  // the 16 MFMAs of a half at in-group half-step c_ (A blocks [m0, m1))
#define Q8_MFMA(FR, c_, m0, m1, STAG)                                                          \
  do {                                                                                         \
    _Pragma("unroll") for (int m = m0; m < m1; m++)                                            \
      _Pragma("unroll") for (int nn = 0; nn < 4; nn++) {                                       \
        if ((STAG) && ((c_) % FCYC) == ((m * 4 + nn) * FCYC) / 16) {                           \
          _Pragma("unroll") for (int r = 0; r < 4; r++) iacc[m][nn][r] += (int32_t)acc[m][nn][r]; \
          acc[m][nn] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_bf16x8(FR[m]), as_bf16x8(FR[4 + nn]), \
                                                               zero4, 0, 0, 0);                \
        } else {                                                                               \
          acc[m][nn] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_bf16x8(FR[m]), as_bf16x8(FR[4 + nn]), \
                                                               acc[m][nn], 0, 0, 0);           \
        }                                                                                      \
      }                                                                                        \
  } while (0)
  // vmcnt before barrier 1 of step st: (st, half 1) landed; younger: (st+1, *), (st+2, *)
#define Q8_VM1(st_, COND)                                                                      \
  do {                                                                                        \
    if (!(COND) || (st_) + 2 < s1) Q8_WAIT_VM(12);                                             \
    else if ((st_) + 1 < s1) Q8_WAIT_VM(6);                                                    \
    else Q8_WAIT_VM(0);                                                                        \
  } while (0)
  // before barrier 2: (st+1, half 0) landed; younger: (st+1, 1), (st+2, *), (st+3, 0)
#define Q8_VM2(st_, COND)                                                                      \
  do {                                                                                        \
    if (!(COND) || (st_) + 3 < s1) Q8_WAIT_VM(12);                                             \
    else if ((st_) + 2 < s1) Q8_WAIT_VM(9);                                                    \
    else if ((st_) + 1 < s1) Q8_WAIT_VM(3);                                                    \
    else Q8_WAIT_VM(0);                                                                        \
  } while (0)
  // K-step st_ in ring slot SL, in-group index q_: F0 holds (in flight) its
  // half 0 on entry and the next step's half 0 on exit.  Barrier 1: every wave
  // has read half 0 (refilled with st+3) and (st, 1) is visible; barrier 2:
  // every wave has read half 1 and (st+1, 0) is visible.
#define Q8_STEP(st_, q_, SL, STAG, COND)                                                       \
  do {                                                                                        \
    Q8_WAIT_LGKM(0); Q8_VM1(st_, COND);                                                        \
    __builtin_amdgcn_s_barrier(); Q8_SB();                                                     \
    if (!(COND) || (st_) + 3 < s1) Q8_ISSUE((st_) + 3, 0, SL);                                 \
    Q8_READ(F1, SL, 1);                                                                        \
    Q8_SB();                                                                                   \
    Q8_MFMA(F0, 2 * (q_), 0, 4, STAG); Q8_SB();                                                \
    Q8_WAIT_LGKM(0); Q8_VM2(st_, COND);                                                        \
    __builtin_amdgcn_s_barrier(); Q8_SB();                                                     \
    if (!(COND) || (st_) + 3 < s1) Q8_ISSUE((st_) + 3, 1, SL);                                 \
    if (!(COND) || (st_) + 1 < s1) Q8_READ(F0, ((SL) + 1) % 3, 0);                             \
    Q8_SB();                                                                                   \
    Q8_MFMA(F1, 2 * (q_) + 1, 0, 4, STAG); Q8_SB();                                            \
  } while (0)
#define Q8_FLUSH()                                                                             \
  do {                                                                                        \
    _Pragma("unroll") for (int a = 0; a < 4; a++)                                              \
      _Pragma("unroll") for (int b = 0; b < 4; b++)                                            \
        _Pragma("unroll") for (int r = 0; r < 4; r++) {                                        \
          iacc[a][b][r] += (int32_t)acc[a][b][r];                                              \
          acc[a][b][r] = 0.0f;                                                                 \
        }                                                                                      \
  } while (0)

  if (s0 >= s1) return;
  Q8_ISSUE(s0, 0, 0);
  Q8_ISSUE(s0, 1, 0);
  if (s0 + 1 < s1) { Q8_ISSUE(s0 + 1, 0, 1); Q8_ISSUE(s0 + 1, 1, 1); }
  if (s0 + 2 < s1) { Q8_ISSUE(s0 + 2, 0, 2); Q8_ISSUE(s0 + 2, 1, 2); }
  // (s0, half 0) landed; younger: (s0, 1) and the two next steps
  if (s0 + 2 < s1) Q8_WAIT_VM(15);
  else if (s0 + 1 < s1) Q8_WAIT_VM(9);
  else Q8_WAIT_VM(3);
  __builtin_amdgcn_s_barrier();
  Q8_SB();
  Q8_READ(F0, 0, 0);
  int64_t st = s0;
  const int64_t sfull = s0 + ((s1 - s0) / 6) * 6;
  for (; st < sfull && st + 8 < s1; st += 6) {
    Q8_STEP(st, 0, 0, 1, 0);
    Q8_STEP(st + 1, 1, 1, 1, 0);
    Q8_STEP(st + 2, 2, 2, 1, 0);
    Q8_STEP(st + 3, 3, 0, 1, 0);
    Q8_STEP(st + 4, 4, 1, 1, 0);
    Q8_STEP(st + 5, 5, 2, 1, 0);
  }
  for (; st < sfull; st += 6) {
    Q8_STEP(st, 0, 0, 1, 1);
    Q8_STEP(st + 1, 1, 1, 1, 1);
    Q8_STEP(st + 2, 2, 2, 1, 1);
    Q8_STEP(st + 3, 3, 0, 1, 1);
    Q8_STEP(st + 4, 4, 1, 1, 1);
    Q8_STEP(st + 5, 5, 2, 1, 1);
  }
  Q8_FLUSH();
  for (int t = 0; st < s1; st++, t++) {
    const int sl = (int)((st - s0) % 3);
    if (sl == 0) Q8_STEP(st, 0, 0, 0, 1);
    else if (sl == 1) Q8_STEP(st, 0, 1, 0, 1);
    else Q8_STEP(st, 0, 2, 0, 1);
    if (FL == 2 && t == 2) Q8_FLUSH();
  }
  Q8_FLUSH();
#undef Q8_WAIT_VM
#undef Q8_WAIT_LGKM
#undef Q8_SB
#undef Q8_ISSUE
#undef Q8_READ
#undef Q8_MFMA
#undef Q8_VM1
#undef Q8_VM2
#undef Q8_STEP
#undef Q8_FLUSH
}

// Drain the 16x16-layout int32 tile into the int64 Gram (row = 4 (lane >> 4) + r,
// col = lane & 15 within each 16x16 block: 4 rows x 128 B per wave-instruction).
__device__ __forceinline__ void g8q_atomics(int32_t (&iacc)[4][4][4], int I, int tj, int64_t np_,
                                            unsigned long long *__restrict__ gram) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wr = wave >> 1, wc = wave & 1;
#pragma unroll
  for (int a = 0; a < 4; a++)
#pragma unroll
    for (int b = 0; b < 4; b++)
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int row = I * BM3 + wr * 64 + a * 16 + 4 * (lane >> 4) + r;
        const int col = tj * BN3 + wc * 64 + b * 16 + (lane & 15);
        const int32_t v = iacc[a][b][r];
        if (v != 0) atomicAdd(gram + (int64_t)row * np_ + col, (unsigned long long)(long long)v);
        iacc[a][b][r] = 0;
      }
}

// The same drain with 512-B row segments: per (a, r) the four 16x16 blocks'
// registers are transposed across the wave's four 16-lane groups (a 4x4
// transpose of (lane group, block): two exchange stages, lanes xor 32 then
// xor 16, two shuffles each), after which register b of lane l holds row
// 16 a + 4 b + r, column 64 wc + l -- one wave-instruction covers one row's 64
// consecutive int64 (4 rows x 128 B before).  The same 64 atomics per wave.
__device__ __forceinline__ void g8q_atomics_wide(int32_t (&iacc)[4][4][4], int I, int tj, int64_t np_,
                                                 unsigned long long *__restrict__ gram) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  const bool g1 = (lane >> 5) & 1, g0 = (lane >> 4) & 1;
#pragma unroll
  for (int a = 0; a < 4; a++)
#pragma unroll
    for (int r = 0; r < 4; r++) {
      int32_t v[4] = {iacc[a][0][r], iacc[a][1][r], iacc[a][2][r], iacc[a][3][r]};
      // stage 1: swap bit 1 of the lane group with bit 1 of the block index
#pragma unroll
      for (int j = 0; j < 2; j++) {
        const int32_t snd = g1 ? v[j] : v[j | 2];
        const int32_t rcv = __shfl_xor(snd, 32, 64);
        if (g1) v[j] = rcv; else v[j | 2] = rcv;
      }
      // stage 2: bit 0 with bit 0
#pragma unroll
      for (int j = 0; j < 4; j += 2) {
        const int32_t snd = g0 ? v[j] : v[j | 1];
        const int32_t rcv = __shfl_xor(snd, 16, 64);
        if (g0) v[j] = rcv; else v[j | 1] = rcv;
      }
      const int col = tj * BN3 + wc * 64 + lane;
#pragma unroll
      for (int b = 0; b < 4; b++) {
        const int row = I * BM3 + wr * 64 + a * 16 + 4 * b + r;
        if (v[b] != 0) atomicAdd(gram + (int64_t)row * np_ + col, (unsigned long long)(long long)v[b]);
      }
#pragma unroll
      for (int b = 0; b < 4; b++) iacc[a][b][r] = 0;
    }
}

// kx = the number of K-ranges the XCDs split the K axis into (8, 4, 2 or 1):
// XCD x runs K-range x % kx of the tile groups g = x / kx (mod 8 / kx).  A
// small cohort (fewer tile groups than XCDs) splits K eight ways; a large one
// gives every XCD whole tile groups over the full K range, so each output tile
// is flushed with int64 atomics only once per int32-exact unit (sps_max steps).
// MODE 0 production; 9 the compile-only no-flush skeleton of GRID_ISA_PROBE.
// LAY 1: row-major panel, quad-row ring (g8_run); K-blocked panel (BL): LAY 3
// the half-split ring with 32x32x16 MFMAs (g8h_run), LAY 4 with 16x16x32 (g8q_run).
template <int MODE, bool BL, int FL, int LAY>
__global__ __launch_bounds__(512, 1) void k_gram8(const uint16_t *__restrict__ z, int64_t ld,
                                                  const int32_t *__restrict__ tiles, int ntiles, int kc, int kx,
                                                  int64_t nsteps, int lag, int spin_ticks,
                                                  int64_t np_, unsigned long long *__restrict__ gram,
                                                  unsigned *__restrict__ rounds, int dyn,
                                                  int32_t *__restrict__ part, GramXoff xoff, int gs) {
  static_assert(MODE == 0 || MODE == 9, "MODE 9 is the no-flush ISA probe");
  static_assert((LAY == 1 && !BL) || ((LAY == 3 || LAY == 4) && BL), "LAY 1: row-major; LAY 3, 4: K-blocked");
  __shared__ __attribute__((aligned(1024))) char smem[3 * SLOT3];
  __shared__ int64_t s_unit;
  const int nwg = gridDim.x;
  const int bid = blockIdx.x;
  const int xcd = bid & 7, l = bid >> 3;
  const int per = nwg >> 3;                       // workgroups per XCD (grid is a multiple of 8)
  const int kr = xcd % kx, gx = 8 / kx, xg = xcd / kx;
  const int64_t xs0 = nsteps * kr / kx, xs1 = nsteps * (kr + 1) / kx;
  const int64_t xlen = xs1 - xs0;
  // this XCD's tile groups of gs tiles (gs = per unless a small cohort deals
  // one group to every XCD): g = xg, xg + gx, ...; only the last group overall
  // can be partial, so every group but this XCD's last holds gs * kc units
  const int64_t ngroups = ((int64_t)ntiles + gs - 1) / gs;
  const int64_t ngx = ngroups > xg ? (ngroups - xg + gx - 1) / gx : 0;
  const int64_t glast = xg + (ngx - 1) * gx;
  const int64_t lastsz = ngx > 0 ? min((int64_t)gs, (int64_t)ntiles - glast * gs) : 0;
  const int64_t units = ngx > 0 ? ((ngx - 1) * gs + lastsz) * kc : 0;
  // dyn: the XCD's workgroups take units in order from a counter instead of
  // unit r * per + l in round r, so a workgroup that starts late (its CU still
  // running the phasing lane's kernel) takes fewer units instead of holding
  // the launch open for its fixed share
  for (int64_t r = 0;; r++) {
    int64_t u = r * per + l;
    if (dyn & 1) {
      if (threadIdx.x == 0)
        s_unit = (int64_t)__hip_atomic_fetch_add(rounds + 128 + xcd * 16, 1u, __ATOMIC_RELAXED,
                                                 __HIP_MEMORY_SCOPE_AGENT);
      __syncthreads();
      u = s_unit;
    }
    if (u >= units) break;
    const int64_t ru = u / per;                     // the unit's round (pacing)
    // unit -> (group, chunk, tile)
    const int64_t gl = u / ((int64_t)gs * kc);
    const int64_t gbase = (xg + gl * gx) * gs;
    const int gsz = (int)min((int64_t)gs, (int64_t)ntiles - gbase);
    const int64_t v = u - gl * (int64_t)gs * kc;
    const int c = (int)(v / gsz);
    const int t = (int)(gbase + v % gsz);
    const int32_t tv = tiles[t];
    // wave-uniform values the compiler cannot prove uniform (u may come from
    // LDS): readfirstlane keeps them, and the K-loop bounds, in SGPRs
    const int I = __builtin_amdgcn_readfirstlane(tv >> 16);
    const int tj = __builtin_amdgcn_readfirstlane(tv & 0xFFFF);
    const int64_t s0 = uniform64(xs0 + xlen * c / kc), s1 = uniform64(xs0 + xlen * (c + 1) / kc);
    // pace: wait (bounded) until the XCD's round ru - lag is complete
    if (ru >= lag && threadIdx.x == 0) {
      const unsigned need = (unsigned)((ru - lag + 1) * per);
      const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
      while (__hip_atomic_load(rounds + xcd * 16, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < need) {
        __builtin_amdgcn_s_sleep(2);
        if (__builtin_amdgcn_s_memrealtime() - t0 > (uint64_t)spin_ticks) break;
      }
    }
    __syncthreads();
    if constexpr (LAY == 4) {
      if (s1 > s0) {
        f32x4 acc[4][4];
        int32_t iacc[4][4][4];
#pragma unroll
        for (int a = 0; a < 4; a++)
#pragma unroll
          for (int b = 0; b < 4; b++)
#pragma unroll
            for (int r = 0; r < 4; r++) { acc[a][b][r] = 0.0f; iacc[a][b][r] = 0; }
        g8q_run<FL>(z, ld, I, tj, s0, s1, smem, acc, iacc);
        if constexpr (MODE != 9) {
          if (dyn & 2) g8q_atomics_wide(iacc, I, tj, np_, gram);
          else g8q_atomics(iacc, I, tj, np_, gram);
        }
      }
    } else if (s1 > s0) {
      f32x16 acc[2][2];
      int32_t iacc[2][2][16];
      g6_zero<2>(acc, iacc);
      if constexpr (LAY == 3) g8h_run<FL>(z, ld, I, tj, s0, s1, smem, acc, iacc);
      else g8_run<FL>(z, ld, I, tj, s0, s1, smem, acc, iacc);
      if constexpr (MODE == 9) {
        // no-flush ISA probe (compile-only, tools/isa_barriers.py --probe): the
        // tile's results are dropped, so every MFMA is dead code
      } else if (part) {
        g8_store_part<2>(iacc, part + (xoff.x[xcd] + u) * (int64_t)(BM3 * BN3));
      } else {
        g6_atomics<2>(iacc, I, tj, np_, gram);
      }
    }
    __syncthreads();
    if (threadIdx.x == 0) __hip_atomic_fetch_add(rounds + xcd * 16, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

#ifdef GRID_ISA_PROBE
// Compile-only (never linked into a library): the round-2 no-flush timing probe
// of the half-split ring, rebuilt so its ISA can be compared with the flushing
// k_gram8<0, true, 1, 3> of the same compile (tools/isa_barriers.py --probe).
template __global__ void k_gram8<0, true, 1, 3>(const uint16_t *__restrict__, int64_t, const int32_t *__restrict__,
                                                int, int, int, int64_t, int, int, int64_t,
                                                unsigned long long *__restrict__, unsigned *__restrict__, int,
                                                int32_t *__restrict__, GramXoff, int);
template __global__ void k_gram8<9, true, 1, 3>(const uint16_t *__restrict__, int64_t, const int32_t *__restrict__,
                                                int, int, int, int64_t, int, int, int64_t,
                                                unsigned long long *__restrict__, unsigned *__restrict__, int,
                                                int32_t *__restrict__, GramXoff, int);
#endif

// ---- symmetric completion and row access ------------------------------------
// The Gram kernels write the upper 128-tiles only.  k_mirror fills every 64x64
// block (a, b), a > b, with the transpose of block (b, a) through LDS, so the
// reads and the writes are whole 512-B row segments; afterwards row i of the
// Gram is contiguous, which is what the row top-k and the multi-GPU
// reduce-scatter by row blocks read.
__global__ __launch_bounds__(256) void k_mirror(int64_t *__restrict__ g, int64_t np_) {
  __shared__ int64_t t[64][65];
  const int64_t p = blockIdx.x;                   // strict lower triangle of 64-blocks, row-major
  int64_t a = (int64_t)((sqrt(8.0 * (double)p + 1.0) + 1.0) * 0.5);
  while (a * (a - 1) / 2 > p) a--;
  while ((a + 1) * a / 2 <= p) a++;
  const int64_t b = p - a * (a - 1) / 2;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
#pragma unroll 4
  for (int r = ty; r < 64; r += 4) t[r][tx] = g[(b * 64 + r) * np_ + a * 64 + tx];
  __syncthreads();
#pragma unroll 4
  for (int r = ty; r < 64; r += 4) g[(a * 64 + r) * np_ + b * 64 + tx] = t[tx][r];
}

__global__ void k_diag(const int64_t *__restrict__ g, int64_t np_, int64_t n, int64_t *__restrict__ nrm) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j < n) nrm[j] = g[j * np_ + j];
}

// Neighbour keys: (d2 << 20) | j, unique per row, ordered by (d2, j); j < 2^20.
// GramKey: exact integer d2 = G_ii + G_jj - 2 G_ij from full Gram rows
// (the MFMA path).  Rows of precomputed fp64 d2 (the direct-difference path)
// do not fit such a key: k_topk_d2 below orders them by (all 64 bits, j).
struct GramKey {
  const int64_t *row;
  const int64_t *nrm;
  int64_t gii;
  typedef int64_t out_t;
  __device__ __forceinline__ unsigned long long key(int64_t j) const {
    return ((unsigned long long)(gii + nrm[j] - 2 * row[j]) << 20) | (unsigned long long)j;
  }
  __device__ __forceinline__ void load4(int64_t j, int64_t st, unsigned long long (&kk)[4]) const {
    int64_t gv[4], nv[4];
#pragma unroll
    for (int u = 0; u < 4; u++) { gv[u] = row[j + u * st]; nv[u] = nrm[j + u * st]; }
#pragma unroll
    for (int u = 0; u < 4; u++)
      kk[u] = ((unsigned long long)(gii + nv[u] - 2 * gv[u]) << 20) | (unsigned long long)(j + u * st);
  }
  __device__ __forceinline__ int64_t value(unsigned long long key) const { return (int64_t)(key >> 20); }
};

__device__ __forceinline__ GramKey make_src(const int64_t *rows, int64_t ld, const int64_t *nrm, double,
                                            int64_t orow, int64_t i) {
  return GramKey{rows + orow * ld, nrm, nrm[i]};
}

// Write the ktake smallest keys of row i (ascending in s[0..ktake)) with self
// dropped and the first k kept (find_neighbors.py:216-225).
template <class Src>
__device__ __forceinline__ void topk_emit(const Src &src, const unsigned long long *s, int64_t ktake, int64_t i,
                                          int64_t k, int64_t orow, int32_t *__restrict__ idx,
                                          typename Src::out_t *__restrict__ d2o, int32_t *__restrict__ cnto) {
  int64_t w = 0;
  bool self = false;
  for (int64_t e = 0; e < ktake; e++) {
    const int64_t j = (int64_t)(s[e] & 0xFFFFFull);
    if (j == i && !self) { self = true; continue; }
    if (w < k) {
      idx[orow * k + w] = (int32_t)j;
      d2o[orow * k + w] = src.value(s[e]);
      w++;
    }
  }
  for (int64_t e = w; e < k; e++) {      // unused slots: idx -1, d2 0
    idx[orow * k + e] = -1;
    d2o[orow * k + e] = 0;
  }
  cnto[orow] = (int32_t)w;
}

// Row top-(k+1), k + 1 <= K1 (BASELINE: k = 10): ONE pass over the row.  Every
// lane keeps the K1 smallest keys of its strided share sorted in registers
// (branch-free insertion, taken only when a key beats the lane's largest);
// each wave then extracts its ktake smallest by wave-wide minimum rounds, and
// one lane merges the four waves' sorted lists.
// j0 / raw (the multi-GPU segment path, grid_knn_seg_topk): only columns
// [j0, n) are scanned (rows points j0 elements before the segment row), and
// the ktake smallest packed keys are written to raw[orow][K1] (ascending,
// ~0 padded) instead of the neighbour lists.
template <int K1, class T>
__global__ __launch_bounds__(256) void k_topk_small(const T *__restrict__ rows, int64_t ld,
                                                    const int64_t *__restrict__ nrm, double scale, int64_t n,
                                                    int64_t k, int64_t row0, int32_t *__restrict__ idx,
                                                    void *__restrict__ d2o, int32_t *__restrict__ cnto,
                                                    int64_t j0 = 0, unsigned long long *__restrict__ raw = nullptr) {
  __shared__ unsigned long long s_w[4][K1];
  __shared__ unsigned long long s_m[4 * K1];
  const int64_t orow = blockIdx.x, i = row0 + orow;
  const auto src = make_src(rows, ld, nrm, scale, orow, i);
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int64_t ktake = (k + 1 < n) ? k + 1 : n;
  unsigned long long L[K1];
#pragma unroll
  for (int t = 0; t < K1; t++) L[t] = ~0ull;
  auto insert = [&](unsigned long long key) {
    if (key < L[K1 - 1]) {
#pragma unroll
      for (int t = 0; t < K1; t++) {
        const unsigned long long lo = key < L[t] ? key : L[t];
        key = key < L[t] ? L[t] : key;
        L[t] = lo;
      }
    }
  };
  int64_t j = j0 + tid;
  for (; j + 3 * 256 < n; j += 4 * 256) {       // four loads of each kind in flight
    unsigned long long kk[4];
    src.load4(j, 256, kk);
#pragma unroll
    for (int u = 0; u < 4; u++) insert(kk[u]);
  }
  for (; j < n; j += 256) insert(src.key(j));
  // wave: the ktake smallest of its 64 sorted lists, ascending
  for (int64_t e = 0; e < ktake; e++) {
    unsigned long long m = L[0];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const unsigned long long x = __shfl_xor(m, o, 64);
      m = x < m ? x : m;
    }
    if (lane == 0) s_w[wv][e] = m;
    const bool pop = L[0] == m;                  // keys are unique: one lane (or none once exhausted)
#pragma unroll
    for (int t = 0; t + 1 < K1; t++) L[t] = pop ? L[t + 1] : L[t];
    L[K1 - 1] = pop ? ~0ull : L[K1 - 1];
  }
  __syncthreads();
  if (tid == 0) {
    int p[4] = {0, 0, 0, 0};
    for (int64_t e = 0; e < ktake; e++) {
      int bw = 0;
      unsigned long long bv = ~0ull;
#pragma unroll
      for (int w = 0; w < 4; w++) {
        const unsigned long long v = p[w] < ktake ? s_w[w][p[w]] : ~0ull;
        if (v < bv) { bv = v; bw = w; }
      }
      p[bw]++;
      s_m[e] = bv;
    }
    if (raw) {
      for (int e = 0; e < K1; e++) raw[orow * K1 + e] = e < ktake ? s_m[e] : ~0ull;
    } else {
      topk_emit(src, s_m, ktake, i, k, orow, idx, (typename decltype(src)::out_t *)d2o, cnto);
    }
  }
}

// ---- multi-GPU: neighbour candidates from upper-triangle row SEGMENTS -------
// A sharded run reduce-scatters only segment b = Gram rows [b*B, (b+1)*B) x
// columns [b*B, np) of the 2W row blocks (rank r: blocks r and 2W-1-r, equal
// volumes), about half of the full rows.  Every pair (i, j) lies in some
// segment: in block(i)'s segment when j >= block(i)*B, else in block(j)'s at
// (row j, column i).  So the true k+1 nearest of row i are among (a) the
// k+1 smallest of row i in its own segment (k_topk_small in raw mode) and
// (b) for every block b <= block(i), the k+1 smallest of COLUMN i in segment
// b (k_seg_cols); k_seg_merge picks them exactly by the packed (d2, j) key.
//
// Column candidates: 32 columns x 8 row groups per workgroup; thread (g, c)
// scans the rows u = g, g + 8, ... (i = r0 + u < n) of column t (j = c0 + t
// < n) keeping the K1 smallest keys (d2 << 20 | i) sorted in registers, and
// one thread per column merges the 8 sorted lists (keys are unique: distinct
// i).  raw[t][K1] ascending, ~0 padded.
template <int K1>
__global__ __launch_bounds__(256) void k_seg_cols(const int64_t *__restrict__ seg, int64_t ld, int64_t nrows,
                                                  int64_t ncols, const int64_t *__restrict__ nrm, int64_t n,
                                                  int64_t r0, int64_t c0, unsigned long long *__restrict__ raw) {
  __shared__ unsigned long long s_l[8][32][K1];
  const int c = threadIdx.x & 31, g = threadIdx.x >> 5;
  const int64_t t = (int64_t)blockIdx.x * 32 + c;
  const int64_t j = c0 + t;
  unsigned long long L[K1];
#pragma unroll
  for (int e = 0; e < K1; e++) L[e] = ~0ull;
  if (t < ncols && j < n) {
    const int64_t gjj = nrm[j];
    const int64_t ue = n - r0 < nrows ? n - r0 : nrows;
    for (int64_t u = g; u < ue; u += 8) {
      const int64_t i = r0 + u;
      unsigned long long key = ((unsigned long long)(nrm[i] + gjj - 2 * seg[u * ld + t]) << 20) |
                               (unsigned long long)i;
      if (key < L[K1 - 1]) {
#pragma unroll
        for (int e = 0; e < K1; e++) {
          const unsigned long long lo = key < L[e] ? key : L[e];
          key = key < L[e] ? L[e] : key;
          L[e] = lo;
        }
      }
    }
  }
#pragma unroll
  for (int e = 0; e < K1; e++) s_l[g][c][e] = L[e];
  __syncthreads();
  if (g == 0 && t < ncols) {
    int p[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int e = 0; e < K1; e++) {
      int bw = 0;
      unsigned long long bv = ~0ull;
#pragma unroll
      for (int w = 0; w < 8; w++) {
        const unsigned long long v = p[w] < K1 ? s_l[w][c][p[w]] : ~0ull;
        if (v < bv) { bv = v; bw = w; }
      }
      p[bw]++;
      raw[t * K1 + e] = bv;
    }
  }
}

// Row i (one thread): the union of its row list (rowc[block(i)][i - block*B])
// and the column lists colc[b][i - b*B] of every block b <= block(i), equal
// keys once (a pair of the diagonal block is in both), the ktake smallest,
// then topk_emit (self dropped, first k kept) -- the rows' top-k exactly as
// k_topk_small on full rows.
template <int K1>
__global__ __launch_bounds__(256) void k_seg_merge(const unsigned long long *__restrict__ rowc,
                                                   const unsigned long long *__restrict__ colc, int64_t ldc,
                                                   int64_t B, int64_t n, int64_t k, int32_t *__restrict__ idx,
                                                   int64_t *__restrict__ d2o, int32_t *__restrict__ cnto) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t ktake = (k + 1 < n) ? k + 1 : n;
  const int64_t bi = i / B;
  unsigned long long L[K1];
#pragma unroll
  for (int e = 0; e < K1; e++) L[e] = ~0ull;
  auto insert = [&](unsigned long long key) {
    if (key < L[K1 - 1]) {
      bool dup = false;
#pragma unroll
      for (int e = 0; e < K1; e++) dup |= L[e] == key;
      if (dup) return;
#pragma unroll
      for (int e = 0; e < K1; e++) {
        const unsigned long long lo = key < L[e] ? key : L[e];
        key = key < L[e] ? L[e] : key;
        L[e] = lo;
      }
    }
  };
  const unsigned long long *rl = rowc + i * K1;        // block-major rows = global row order
  for (int e = 0; e < K1; e++) insert(rl[e]);
  for (int64_t b = 0; b <= bi; b++) {
    const unsigned long long *cl = colc + (b * ldc + (i - b * B)) * K1;
    for (int e = 0; e < K1; e++) insert(cl[e]);
  }
  int64_t w = 0;
  bool self = false;
  for (int64_t e = 0; e < ktake; e++) {
    const unsigned long long key = L[e];
    const int64_t j = (int64_t)(key & 0xFFFFFull);
    if (j == i && !self) { self = true; continue; }
    if (w < k) {
      idx[i * k + w] = (int32_t)j;
      d2o[i * k + w] = (int64_t)(key >> 20);
      w++;
    }
  }
  for (int64_t e = w; e < k; e++) {
    idx[i * k + e] = -1;
    d2o[i * k + e] = 0;
  }
  cnto[i] = (int32_t)w;
}

// k_seg_merge with one WAVE per row (round 6: the thread-per-row form kept 13
// workgroups busy at n = 3,202 and walked up to 2W + 1 lists of K1 keys
// serially, 122 us per step at W = 8): the row's T = K1 (bi + 2) candidate keys
// are spread over the lanes (R per lane), then the k + 1 smallest DISTINCT
// keys are taken one by one by wave minima (equal keys -- a pair seen as a row
// and as a column entry -- once), then the same self-drop and first-k rule.
template <int K1, int R>
__global__ __launch_bounds__(256) void k_seg_merge_w(const unsigned long long *__restrict__ rowc,
                                                     const unsigned long long *__restrict__ colc, int64_t ldc,
                                                     int64_t B, int64_t n, int64_t k, int32_t *__restrict__ idx,
                                                     int64_t *__restrict__ d2o, int32_t *__restrict__ cnto) {
  const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (i >= n) return;                                  // whole waves leave together
  const int64_t ktake = (k + 1 < n) ? k + 1 : n;
  const int64_t bi = i / B;
  const int64_t T = (int64_t)K1 * (bi + 2);
  unsigned long long v[R];
#pragma unroll
  for (int r = 0; r < R; r++) {
    const int64_t t = lane + 64 * r;
    unsigned long long key = ~0ull;
    if (t < K1) {
      key = rowc[i * K1 + t];
    } else if (t < T) {
      const int64_t b = (t - K1) / K1, e = (t - K1) % K1;
      key = colc[(b * ldc + (i - b * B)) * K1 + e];
    }
    v[r] = key;
  }
  int64_t w = 0;
  bool self = false;
  for (int64_t e = 0; e < ktake; e++) {
    unsigned long long m = v[0];
#pragma unroll
    for (int r = 1; r < R; r++) m = v[r] < m ? v[r] : m;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const unsigned long long y = __shfl_xor(m, o, 64);
      m = y < m ? y : m;
    }
    if (m == ~0ull) break;
#pragma unroll
    for (int r = 0; r < R; r++) v[r] = v[r] == m ? ~0ull : v[r];
    const int64_t j = (int64_t)(m & 0xFFFFFull);
    if (j == i && !self) {
      self = true;
      continue;
    }
    if (w < k) {
      if (lane == 0) {
        idx[i * k + w] = (int32_t)j;
        d2o[i * k + w] = (int64_t)(m >> 20);
      }
      w++;
    }
  }
  if (lane == 0) {
    for (int64_t e = w; e < k; e++) {
      idx[i * k + e] = -1;
      d2o[i * k + e] = 0;
    }
    cnto[i] = (int32_t)w;
  }
}

// the bin split's send buffer: blockIdx.y = 2 q + slot (block b = q or
// 2W-1-q), blockIdx.x = row r of the block; one coalesced row copy each
__global__ __launch_bounds__(256) void k_seg_pack(const int64_t *__restrict__ gram, int64_t np_, int64_t W, int64_t B,
                                                  int64_t *__restrict__ send) {
  const int64_t q = blockIdx.y >> 1, slot = blockIdx.y & 1, r = blockIdx.x;
  const int64_t b = slot ? 2 * W - 1 - q : q;
  const int64_t nc = (2 * W - b) * B;
  const int64_t off = q * B * (2 * W + 1) * B + (slot ? B * (2 * W - q) * B : 0);
  int64_t *dst = send + off + r * nc;
  const int64_t row = b * B + r;
  const int64_t c0 = b * B;
  for (int64_t c = threadIdx.x; c < nc; c += blockDim.x) {
    const int64_t col = c0 + c;
    dst[c] = (row < np_ && col < np_) ? gram[row * np_ + col] : 0;
  }
}

// ---- complete rows from the segments (k + 1 > GRID_SEG_K1) -------------------
// Row block b lacks columns [0, b B): for b' < b that part is the transposed
// tile T(b', b)[u][c] = seg_b'[c][(b - b') B + u], held by rank own(b').  THE
// exchange rule (include/grid_abi.h): rank own(b') sends T(b', b) to rank
// own(b) in this slot of the pair's two.  With p = own(b'), q = own(b):
// p < q carries T(p, q) and T(p, 2W-1-q), p > q carries T(p, 2W-1-q) and
// T(2W-1-p, 2W-1-q), p = q only T(p, 2W-1-p).
__host__ __device__ __forceinline__ int64_t seg_own(int64_t b, int64_t W) { return b < W ? b : 2 * W - 1 - b; }
__host__ __device__ __forceinline__ int64_t seg_tile_slot(int64_t bs, int64_t b, int64_t W) {
  const int64_t p = seg_own(bs, W), q = seg_own(b, W);
  if (p < q) return b < W ? 0 : 1;
  if (p > q) return bs < W ? 0 : 1;
  return 0;
}

// One 32x32 int64 sub-tile per workgroup through LDS: blockIdx.z = tile
// (b = bs + 1 + z), blockIdx.x / .y = the sub-tile's u / c origin.  Reads run
// along segment rows and writes along tile rows (256-B runs both); the LDS
// rows are padded by one 8-byte element, so the 16-lane write groups fill 32
// distinct banks and the 32-lane transposed reads 64.  Cells beyond B (the
// last sub-tile in each direction) are neither read nor written.
__global__ __launch_bounds__(256) void k_seg_tiles_pack(const int64_t *__restrict__ seg, int64_t ld, int64_t B,
                                                        int64_t W, int64_t bs, int64_t *__restrict__ send) {
  __shared__ int64_t t[32][33];
  const int64_t b = bs + 1 + blockIdx.z;
  const int64_t u0 = (int64_t)blockIdx.x * 32, c0 = (int64_t)blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int64_t *src = seg + (b - bs) * B;
#pragma unroll
  for (int r = ty; r < 32; r += 8) {
    const int64_t c = c0 + r, u = u0 + tx;
    if (c < B && u < B) t[r][tx] = src[c * ld + u];
  }
  __syncthreads();
  int64_t *dst = send + (2 * seg_own(b, W) + seg_tile_slot(bs, b, W)) * B * B;
#pragma unroll
  for (int r = ty; r < 32; r += 8) {
    const int64_t u = u0 + r, c = c0 + tx;
    if (u < B && c < B) dst[u * B + c] = t[tx][r];
  }
}

// blockIdx.x = row u of block b, blockIdx.y = column block b': one coalesced
// copy of B cells, from the received tile T(b', b) for b' < b, else from the
// block's own segment
__global__ __launch_bounds__(256) void k_seg_rows_fill(const int64_t *__restrict__ seg, int64_t ld,
                                                       const int64_t *__restrict__ recv, int64_t B, int64_t W,
                                                       int64_t b, int64_t *__restrict__ rows, int64_t ld_rows) {
  const int64_t u = blockIdx.x, bs = blockIdx.y;
  const int64_t *src = bs < b ? recv + ((2 * seg_own(bs, W) + seg_tile_slot(bs, b, W)) * B + u) * B
                              : seg + u * ld + (bs - b) * B;
  int64_t *dst = rows + u * ld_rows + bs * B;
  for (int64_t c = threadIdx.x; c < B; c += blockDim.x) dst[c] = src[c];
}

// Row top-(k+1) for larger k: 8-pass radix select on the packed keys over the
// (coalesced) row, then a bitonic sort of the <= SELCAP survivors.
constexpr int SELCAP = 4096;

template <class T>
__global__ __launch_bounds__(256) void k_topk_radix(const T *__restrict__ rows, int64_t ld,
                                                    const int64_t *__restrict__ nrm, double scale, int64_t n,
                                                    int64_t k, int64_t row0, int32_t *__restrict__ idx,
                                                    void *__restrict__ d2o, int32_t *__restrict__ cnto,
                                                    int64_t = 0, unsigned long long *__restrict__ = nullptr) {
  __shared__ unsigned hist[256];
  __shared__ unsigned long long s_prefix;
  __shared__ long long s_rank;
  __shared__ unsigned long long sel[SELCAP];
  __shared__ int s_nsel;
  const int64_t orow = blockIdx.x, i = row0 + orow;
  const auto src = make_src(rows, ld, nrm, scale, orow, i);
  const int tid = threadIdx.x;
  const int64_t ktake = (k + 1 < n) ? k + 1 : n;
  unsigned long long prefix = 0, mask = 0;
  long long rank = ktake - 1;
  for (int shift = 56; shift >= 0; shift -= 8) {
    hist[tid] = 0;
    __syncthreads();
    for (int64_t j = tid; j < n; j += 256) {
      const unsigned long long kk = src.key(j);
      if ((kk & mask) == prefix) atomicAdd(&hist[(kk >> shift) & 255], 1u);
    }
    __syncthreads();
    if (tid == 0) {
      long long cum = 0;
      for (int d = 0; d < 256; d++) {
        if (cum + hist[d] > rank) {
          s_prefix = prefix | ((unsigned long long)d << shift);
          s_rank = rank - cum;
          break;
        }
        cum += hist[d];
      }
    }
    __syncthreads();
    prefix = s_prefix;
    rank = s_rank;
    mask |= 0xFFull << shift;
    __syncthreads();
  }
  const unsigned long long T_ = prefix;   // the ktake-th smallest key (keys unique)
  if (tid == 0) s_nsel = 0;
  for (int e = tid; e < SELCAP; e += 256) sel[e] = ~0ull;
  __syncthreads();
  for (int64_t j = tid; j < n; j += 256) {
    const unsigned long long kk = src.key(j);
    if (kk <= T_) {
      const int p = atomicAdd(&s_nsel, 1);
      if (p < SELCAP) sel[p] = kk;
    }
  }
  __syncthreads();
  int cap = 1;
  while (cap < ktake) cap <<= 1;
  for (int size = 2; size <= cap; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int e = tid; e < cap; e += 256) {
        const int p = e ^ stride;
        if (p > e) {
          const bool up = (e & size) == 0;
          const unsigned long long a = sel[e], b = sel[p];
          if ((a > b) == up) { sel[e] = b; sel[p] = a; }
        }
      }
      __syncthreads();
    }
  }
  if (tid == 0) topk_emit(src, sel, ktake, i, k, orow, idx, (typename decltype(src)::out_t *)d2o, cnto);
}

// Row top-(k+1) of precomputed fp64 distances, ordered EXACTLY by (d2, j): a
// non-negative double orders as its bit pattern, so the selection is a radix
// select over the 64 value bits (8 passes; -0.0 counts as +0.0), then, only
// when the (k+1)-th smallest value is shared by entries on both sides of the
// boundary, over the 24 index bits of the entries with that value (3 passes);
// the survivors -- exactly ktake -- are sorted as (bits, j) pairs.  No key is
// shortened, so distances that differ in their last bit are told apart
// whatever the largest distance of the matrix is.
__global__ __launch_bounds__(256) void k_topk_d2(const double *__restrict__ rows, int64_t ld, int64_t n, int64_t k,
                                                 int64_t row0, int32_t *__restrict__ idx, double *__restrict__ d2o,
                                                 int32_t *__restrict__ cnto) {
  __shared__ unsigned hist[256];
  __shared__ unsigned long long s_prefix;
  __shared__ long long s_rank;
  __shared__ unsigned s_cnt;
  __shared__ int s_nsel;
  __shared__ unsigned long long sel_v[SELCAP];
  __shared__ int32_t sel_j[SELCAP];
  const int64_t orow = blockIdx.x, i = row0 + orow;
  const double *row = rows + orow * ld;
  const int tid = threadIdx.x;
  const int64_t ktake = (k + 1 < n) ? k + 1 : n;
  auto bits = [&](int64_t j) { return (unsigned long long)__double_as_longlong(row[j] + 0.0); };
  // digit d of the bucket holding rank `rank`; the rank inside it
  auto pick = [&](unsigned long long prefix, long long rank, int shift) {
    long long cum = 0;
    for (int d = 0; d < 256; d++) {
      if (cum + hist[d] > rank) {
        s_prefix = prefix | ((unsigned long long)d << shift);
        s_rank = rank - cum;
        s_cnt = hist[d];
        break;
      }
      cum += hist[d];
    }
  };
  unsigned long long prefix = 0, mask = 0;
  long long rank = ktake - 1;
  for (int shift = 56; shift >= 0; shift -= 8) {
    hist[tid] = 0;
    __syncthreads();
    for (int64_t j = tid; j < n; j += 256) {
      const unsigned long long b = bits(j);
      if ((b & mask) == prefix) atomicAdd(&hist[(b >> shift) & 255], 1u);
    }
    __syncthreads();
    if (tid == 0) pick(prefix, rank, shift);
    __syncthreads();
    prefix = s_prefix;
    rank = s_rank;
    mask |= 0xFFull << shift;
    __syncthreads();
  }
  const unsigned long long V = prefix;    // the ktake-th smallest value; rank + 1 of its s_cnt entries are taken
  unsigned long long J = 0xFFFFFFull;     // ... those with j <= J
  if ((long long)s_cnt != rank + 1) {
    unsigned long long jp = 0, jm = 0;
    for (int shift = 16; shift >= 0; shift -= 8) {
      __syncthreads();
      hist[tid] = 0;
      __syncthreads();
      for (int64_t j = tid; j < n; j += 256)
        if (bits(j) == V && ((unsigned long long)j & jm) == jp) atomicAdd(&hist[(j >> shift) & 255], 1u);
      __syncthreads();
      if (tid == 0) pick(jp, rank, shift);
      __syncthreads();
      jp = s_prefix;
      rank = s_rank;
      jm |= 0xFFull << shift;
    }
    J = jp;
  }
  __syncthreads();
  if (tid == 0) s_nsel = 0;
  for (int e = tid; e < SELCAP; e += 256) { sel_v[e] = ~0ull; sel_j[e] = 0x7FFFFFFF; }
  __syncthreads();
  for (int64_t j = tid; j < n; j += 256) {
    const unsigned long long b = bits(j);
    if (b < V || (b == V && (unsigned long long)j <= J)) {
      const int p = atomicAdd(&s_nsel, 1);
      if (p < SELCAP) { sel_v[p] = b; sel_j[p] = (int32_t)j; }
    }
  }
  __syncthreads();
  int cap = 1;
  while (cap < ktake) cap <<= 1;
  for (int size = 2; size <= cap; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int e = tid; e < cap; e += 256) {
        const int p = e ^ stride;
        if (p > e) {
          const bool up = (e & size) == 0;
          const unsigned long long a = sel_v[e], b = sel_v[p];
          const int32_t ja = sel_j[e], jb = sel_j[p];
          const bool gt = a > b || (a == b && ja > jb);
          if (gt == up) { sel_v[e] = b; sel_v[p] = a; sel_j[e] = jb; sel_j[p] = ja; }
        }
      }
      __syncthreads();
    }
  }
  if (tid == 0) {                          // topk_emit's rule on the (bits, j) pairs
    int64_t w = 0;
    bool self = false;
    for (int64_t e = 0; e < ktake; e++) {
      const int64_t j = sel_j[e];
      if (j == i && !self) { self = true; continue; }
      if (w < k) {
        idx[orow * k + w] = (int32_t)j;
        d2o[orow * k + w] = __longlong_as_double((long long)sel_v[e]);
        w++;
      }
    }
    for (int64_t e = w; e < k; e++) {
      idx[orow * k + e] = -1;
      d2o[orow * k + e] = 0;
    }
    cnto[orow] = (int32_t)w;
  }
}

// ---- general-value k-NN (values that are not bf16-exact) -----------------
// Panel of the MFMA path from int32 hundredths: K-blocked bf16 of
// clip(zq[i][cols[c]], -qmax, qmax), GRID_MISSING -> 0 (find_neighbors.py:57-58).
// The step-4 output handed over in one process (utils/handoff.py) carries the
// "-0.00" sentinel GRID_ZQ_NEG0: float("-0.00") is -0.0, a zero here.
__global__ void k_panel_i32(const int32_t *__restrict__ zq, int64_t n, int64_t ld, const int32_t *__restrict__ cols,
                            int64_t r, int32_t qmax, uint16_t *__restrict__ zb, int64_t np_, int64_t kpad) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t i = blockIdx.y;
  if (c >= kpad) return;
  int32_t v = 0;
  if (i < n && c < r) {
    v = zq[i * ld + cols[c]];
    v = (v == GRID_MISSING || v == GRID_ZQ_NEG0) ? 0 : min(max(v, -qmax), qmax);   // np.clip: max, then min
  }
  zb[(c / KBW) * np_ * KBW + i * KBW + (c % KBW)] = (uint16_t)(__float_as_uint((float)v) >> 16);
}
// Column gather + clip into a dense [n][r] matrix for the direct-difference
// kernels: int32 hundredths (exact path) or fp64 values clip(q/100, +-zmax)
// (np.clip on float(text) values, :57; NaN -> 0, :58).
__global__ void k_gather_i32(const int32_t *__restrict__ zq, int64_t n, int64_t ld, const int32_t *__restrict__ cols,
                             int64_t r, int32_t qmax, int32_t *__restrict__ out) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t i = blockIdx.y;
  if (c >= r) return;
  const int32_t v = zq[i * ld + cols[c]];
  out[i * r + c] = (v == GRID_MISSING || v == GRID_ZQ_NEG0) ? 0 : min(max(v, -qmax), qmax);
}
__global__ void k_gather_f64(const int32_t *__restrict__ zq, int64_t n, int64_t ld, const int32_t *__restrict__ cols,
                             int64_t r, double zmax, double *__restrict__ out) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t i = blockIdx.y;
  if (c >= r) return;
  const int32_t v = zq[i * ld + cols[c]];
  const double x = v == GRID_ZQ_NEG0 ? -0.0 : (double)v / 100.0; // float("%.2f" text)
  const double lo = -zmax, y = x < lo ? lo : x;                  // np.clip: maximum(x, -zmax) ...
  out[i * r + c] = v == GRID_MISSING ? 0.0 : (y > zmax ? zmax : y);   // ... then minimum(., zmax)
}

// d2[i][j] = sum_k (z_ik - z_jk)^2 for the upper 64-tiles (i-tile <= j-tile),
// sequential over k: exact int64 for integer hundredths (stored as fp64, exact
// below 2^53; the caller checks the bound), a fixed-order fp64 sum (no FMA
// contraction: -ffp-contract=off) for general values.  64x64 tile per
// 256-thread workgroup, 4x4 outputs per thread, 32-column K slabs in LDS.
template <class T, class ACC>
__global__ __launch_bounds__(256) void k_dist(const T *__restrict__ z, int64_t ld, int64_t n, int64_t r,
                                              double *__restrict__ d2, int64_t np_, int64_t nb) {
  __shared__ T As[32][64 + 1], Bs[32][64 + 1];
  int64_t p = blockIdx.x, bi = 0;
  while (p >= nb - bi) { p -= nb - bi; bi++; }
  const int64_t bj = bi + p;
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  ACC acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; a++)
#pragma unroll
    for (int b = 0; b < 4; b++) acc[a][b] = 0;
  for (int64_t k0 = 0; k0 < r; k0 += 32) {
    // 64 rows x 32 columns per operand: thread loads 8 elements of each
#pragma unroll
    for (int u = 0; u < 8; u++) {
      const int e = tid + u * 256, row = e >> 5, kk = e & 31;
      const int64_t ia = bi * 64 + row, ib = bj * 64 + row, kc = k0 + kk;
      As[kk][row] = (ia < n && kc < r) ? z[ia * ld + kc] : (T)0;
      Bs[kk][row] = (ib < n && kc < r) ? z[ib * ld + kc] : (T)0;
    }
    __syncthreads();
#pragma unroll 4
    for (int kk = 0; kk < 32; kk++) {
      T av[4], bv[4];
#pragma unroll
      for (int a = 0; a < 4; a++) av[a] = As[kk][ty * 4 + a];
#pragma unroll
      for (int b = 0; b < 4; b++) bv[b] = Bs[kk][tx * 4 + b];
#pragma unroll
      for (int a = 0; a < 4; a++)
#pragma unroll
        for (int b = 0; b < 4; b++) {
          const ACC d = (ACC)av[a] - (ACC)bv[b];
          acc[a][b] = acc[a][b] + d * d;
        }
    }
    __syncthreads();
  }
#pragma unroll
  for (int a = 0; a < 4; a++)
#pragma unroll
    for (int b = 0; b < 4; b++)
      d2[(bi * 64 + ty * 4 + a) * np_ + bj * 64 + tx * 4 + b] = (double)acc[a][b];
}

}  // namespace

extern "C" {

// Launch k_gram8 (persistent, XCD-paced) over the upper-triangle 256x128
// tiles (I, j >= 2I) with I in [ti0, ti1) -- all of them for the whole Gram,
// one row range for the cohort split's segments (grid_knn_gram_kb_rows);
// tile element (row, col) is added into d_gram[row * ldg + col].  The tile
// lists live in GRID_TILE_SLOTS slots keyed by (np, ti0, ti1), each in its own
// device buffer grown to the list's size, so launches that alternate between
// row ranges re-use their uploaded lists instead of re-uploading them (a host
// sync) every time, and the whole triangle of any np fits.
static int launch_gram8(grid_ctx *ctx, const uint16_t *d_zb, int64_t np_, int64_t nsteps, int64_t ld,
                        int64_t q2, int64_t sps_max, bool blocked, int64_t *d_gram, int ti0, int ti1,
                        int64_t ldg) {
  const int nt = (int)(np_ / BM);
  int nt6 = 0;
  for (int i = ti0; i < ti1; i++) nt6 += nt - 2 * i;
  REQUIRE(nt6 > 0, "empty Gram row range");
  REQUIRE(nt < (1 << 16), "np %lld: tile coordinates exceed 16 bits", (long long)np_);
  int slot = -1, lru = 0;
  for (int s = 0; s < GRID_TILE_SLOTS; s++) {
    const GridTileSlot &c = ctx->tiles[s];
    if (c.np == np_ && c.ti0 == ti0 && c.ti1 == ti1 && c.n == nt6 && c.host && c.dev) slot = s;
    if (c.used < ctx->tiles[lru].used) lru = s;
  }
  if (slot < 0) {
    slot = lru;
    GridTileSlot &ts = ctx->tiles[slot];
    delete[] ts.host;
    ts.host = nullptr;
    ts.np = -1;
    if ((size_t)nt6 > ts.cap) {
      // a launch queued on the stream may still read the slot's old list
      HIPCHK(hipStreamSynchronize(ctx->stream));
      if (ts.dev) HIPCHK(hipFree(ts.dev));
      ts.dev = nullptr;
      ts.cap = 0;
      HIPCHK(hipMalloc((void **)&ts.dev, (size_t)nt6 * 4));
      ts.cap = (size_t)nt6;
    }
    ts.host = new int32_t[nt6];
    // super-block order (groups of GI6 row tiles x GJ6 column tiles, see GI6),
    // enumerated incrementally from the range's first row tile
    int t = 0;
    for (int i0 = ti0; i0 < ti1; i0 += GI6) {
      const int i1 = std::min(ti1, i0 + GI6);
      for (int bj = (2 * i0) / GJ6; bj * GJ6 < nt; bj++) {
        const int j0 = bj * GJ6, j1 = std::min(nt, j0 + GJ6);
        for (int i = i0; i < i1; i++)
          for (int j = std::max(j0, 2 * i); j < j1; j++) ts.host[t++] = (i << 16) | j;
      }
    }
    REQUIRE(t == nt6, "tile enumeration");
    HIPCHK(hipMemcpyAsync(ts.dev, ts.host, (size_t)nt6 * 4, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    ts.np = np_;
    ts.ti0 = ti0;
    ts.ti1 = ti1;
    ts.n = nt6;
  }
  ctx->tiles[slot].used = ++ctx->tiles_clock;
  const int32_t *d_tiles = ctx->tiles[slot].dev;
  unsigned *rounds = (unsigned *)((char *)ctx->aux + GRID_AUX_BYTES / 2);
  HIPCHK(hipMemsetAsync(rounds, 0, (128 + 8 * 16) * 4, ctx->stream));   // round and unit counters
  const int per = ctx->ncu >= 8 ? ctx->ncu / 8 : 1;   // workgroups per XCD
  // tiles per group (tools A/B GRID_GRAM_GS, default per): fewer than per deals
  // a small cohort's tiles to more groups, so that every XCD can take whole
  // groups over the full K range (kx = 1) and all XCDs stream the same K-steps
  int gs = per;
  const char *gse = GRID_AB_KNOB("GRID_GRAM_GS");
  if (gse && atoi(gse) >= 1 && atoi(gse) < per) gs = atoi(gse);
  const int64_t ngroups = ceil_div(nt6, gs);
  // (kx, kc): cost = the longest XCD's sequential work per workgroup in
  // K-step units: rounds x (steps per unit + UF), where UF prices a unit's
  // prologue and its int64-atomic flush (256 KiB per workgroup at ~5 GB/s per
  // CU: ~25-50 us, i.e. tens of K-steps -- without it, short K ranges were cut
  // into hundreds of units and the flushes doubled the launch); the fewest
  // K-ranges within 1 % of the best cost, then the chunk count that wastes least
  const double UF = 40.0;
  int64_t bkx = 8, bkc = 1;
  double bcost = -1.0;
  for (int kx = 8; kx >= 1; kx >>= 1) {
    const int gx = 8 / kx;
    const int64_t xlen = ceil_div(nsteps, kx);
    const int64_t kcmin = ceil_div(xlen, sps_max);
    for (int64_t kc = kcmin; kc < kcmin + 32; kc++) {
      int64_t worst = 0;
      for (int xg = 0; xg < gx; xg++) {
        const int64_t ngx = ngroups > xg ? (ngroups - xg + gx - 1) / gx : 0;
        if (ngx == 0) continue;
        const int64_t glast = xg + (ngx - 1) * gx;
        const int64_t lastsz = std::min((int64_t)gs, (int64_t)nt6 - glast * gs);
        const int64_t units = ((ngx - 1) * gs + lastsz) * kc;
        worst = std::max(worst, ceil_div(units, per));
      }
      const double cost = (double)worst * ((double)ceil_div(xlen, kc) + UF);
      if (bcost < 0 || cost < bcost * 0.99 || (kx < bkx && cost <= bcost * 1.01) ||
          (kx == bkx && cost < bcost)) {
        bcost = cost;
        bkx = kx;
        bkc = kc;
      }
    }
  }
  // performance knobs only (results are exact for any value)
  const char *le = getenv("GRID_GRAM_LAG"), *se = getenv("GRID_GRAM_SPIN"), *ke = getenv("GRID_GRAM_KC");
  const char *xe = getenv("GRID_GRAM_KX");
  const int lag = le ? atoi(le) : 1, spin = se ? atoi(se) : 20000;
  const char *dye = GRID_AB_KNOB("GRID_GRAM_DYN");      // units from a per-XCD counter (1) or fixed per workgroup (0)
  // bit 1: the 16x16 layout's flush in 512-B row segments (g8q_atomics_wide; A/B GRID_GRAM_WIDE)
  const char *wde = GRID_AB_KNOB("GRID_GRAM_WIDE");
  const int dyn = (dye ? atoi(dye) != 0 : 1) | ((wde ? atoi(wde) != 0 : GRAM_WIDE) ? 2 : 0);
  if (xe && (atoi(xe) == 1 || atoi(xe) == 2 || atoi(xe) == 4 || atoi(xe) == 8)) {
    bkx = atoi(xe);
    bkc = ceil_div(ceil_div(nsteps, bkx), sps_max);
  }
  if (ke && atoi(ke) > bkc) bkc = atoi(ke);
  REQUIRE(ceil_div(ceil_div(nsteps, bkx), bkc) <= sps_max, "Gram K chunk exceeds the int32-exact length");
  // fp32 chunks of 384 products while 384 qmax^2 <= 2^24 (qmax <= 209), else 192
  const int fl = 384 * q2 <= (1ll << 24) ? 1 : 2;
  // Row-major panel: the quad-row ring (LAY 1).  K-blocked panel
  // ([kpad/KBW][np][KBW], KBW = 32), half-split ring: 16x16x32 MFMAs (LAY 4) for
  // 384-product fp32 chunks (28.96 vs 29.83 ms at config 2, 887 vs 909 ms at the
  // config-3 chunk, r03ae), 32x32x16 (LAY 3) for FL = 2, where LAY 4's loop spills.
  static_assert(KBW == BK / 2, "k_gram8's K-blocked path reads 32-wide K-blocks");
  auto kern = blocked ? (fl == 1 ? k_gram8<0, true, 1, 4> : k_gram8<0, true, 2, 3>)
                      : (fl == 1 ? k_gram8<0, false, 1, 1> : k_gram8<0, false, 2, 1>);
  const bool q16 = blocked && fl == 1;   // LAY 4: the 16x16 tile has no partial-mode flush
  // partial mode (GRID_GRAM_PART_MB > 0: while the slots fit that many MiB; off by default): plain
  // int32 stores of each unit's tile into its own slot, one reduction launch
  // after the Gram, in place of the int64 atomics (the atomics were not what bounds the Gram)
  const char *pme = GRID_AB_KNOB("GRID_GRAM_PART_MB");
  const int64_t part_cap = (int64_t)(pme ? atof(pme) : 0.0) << 20;   // measured slower: 29.3 vs 28.3 ms at config 2
  int32_t *d_part = nullptr;
  GramXoff xoff{};
  {
    const int gx = 8 / (int)bkx;
    int64_t tot = 0;
    for (int x = 0; x < 8; x++) {
      const int xg = x / (int)bkx;
      const int64_t ngx = ngroups > xg ? (ngroups - xg + gx - 1) / gx : 0;
      const int64_t glast = xg + (ngx - 1) * gx;
      const int64_t lastsz = ngx > 0 ? std::min((int64_t)gs, (int64_t)nt6 - glast * gs) : 0;
      xoff.x[x] = tot;
      tot += ngx > 0 ? ((ngx - 1) * gs + lastsz) * bkc : 0;
    }
    if (!q16 && gs == per && part_cap > 0 && ldg == np_ && ti0 == 0 && tot * (int64_t)(BM3 * BN3 * 4) <= part_cap) {
      void *sp = nullptr;
      int rc = grid_scratch(ctx, (size_t)tot * BM3 * BN3 * 4, &sp);
      if (rc) return rc;
      d_part = (int32_t *)sp;
    }
  }
  hipLaunchKernelGGL(kern, dim3((unsigned)(8 * per)), dim3(512), 0, ctx->stream, d_zb, ld,
                     d_tiles, nt6, (int)bkc, (int)bkx, nsteps, lag, spin, ldg,
                     (unsigned long long *)d_gram, rounds, dyn, d_part, xoff, gs);
  LAUNCHCHK();
  if (d_part) {
    hipLaunchKernelGGL(k_gram_part_reduce, dim3((unsigned)(BM3 * BN3 / 256), (unsigned)nt6), dim3(256), 0,
                       ctx->stream, d_part, xoff, per, (int)bkc, (int)bkx, nsteps, nt6, d_tiles,
                       ldg, d_gram);
    LAUNCHCHK();
  }
  return GRID_OK;
}

int grid_knn_gram(grid_ctx *ctx, const uint16_t *d_zb, int64_t np_, int64_t kpad, int64_t ld,
                  int32_t qmax, int64_t *d_gram) {
  REQUIRE(ctx && d_zb && d_gram, "bad args");
  REQUIRE(np_ > 0 && np_ % BM == 0, "np (%lld) must be a positive multiple of %d", (long long)np_, BM);
  REQUIRE(kpad >= 0 && kpad % BK == 0 && ld >= kpad && ld % 8 == 0, "kpad must be a multiple of %d", BK);
  REQUIRE(((uintptr_t)d_zb % 16) == 0, "zb must be 16-byte aligned");
  REQUIRE(qmax >= 0 && qmax <= 256, "qmax must be in [0, 256]");
  if (kpad == 0) return GRID_OK;
  const int64_t nsteps = kpad / BK;
  const int64_t q2 = (int64_t)(qmax > 0 ? qmax : 1) * (qmax > 0 ? qmax : 1);
  // fp32-exact flush interval and int32-exact slice length, in K-steps
  int fs = (int)((1ll << 24) / (q2 * BK));
  if (fs < 1) fs = 1;
  int64_t sps_max = ((1ll << 31) - 1) / (q2 * BK);
  const int nt = (int)(np_ / BM);
  const int ntiles = nt * (nt + 1) / 2;
  if (np_ % BM3 == 0)
    return launch_gram8(ctx, d_zb, np_, nsteps, ld, q2, sps_max, false, d_gram, 0, (int)(np_ / BM3), np_);
  {
    // np % 256 != 0: 128x128 tiles, one K-slice per workgroup
    int64_t target_slices = ceil_div(2048, ntiles);
    int64_t sps = ceil_div(nsteps, target_slices);
    if (sps > sps_max) sps = sps_max;
    if (sps < 1) sps = 1;
    const int64_t nslices = ceil_div(nsteps, sps);
    const int64_t nwg = nslices * ntiles;
    REQUIRE(nwg < (1ll << 31), "too many work items");
    hipLaunchKernelGGL(k_gram_dma, dim3((unsigned)nwg), dim3(NT), 0, ctx->stream, d_zb, ld, nt, ntiles, nsteps,
                       (int)sps, fs, np_, (unsigned long long *)d_gram);
  }
  LAUNCHCHK();
  return GRID_OK;
}

int grid_knn_gram_kb(grid_ctx *ctx, const uint16_t *d_zb, int64_t np_, int64_t kpad, int32_t qmax,
                     int64_t *d_gram) {
  REQUIRE(ctx && d_zb && d_gram, "bad args");
  REQUIRE(np_ > 0 && np_ % BM3 == 0, "np (%lld) must be a positive multiple of %d", (long long)np_, BM3);
  REQUIRE(kpad >= 0 && kpad % BK == 0, "kpad must be a multiple of %d", BK);
  REQUIRE(((uintptr_t)d_zb % 16) == 0, "zb must be 16-byte aligned");
  REQUIRE(qmax >= 0 && qmax <= 256, "qmax must be in [0, 256]");
  if (kpad == 0) return GRID_OK;
  const int64_t q2 = (int64_t)(qmax > 0 ? qmax : 1) * (qmax > 0 ? qmax : 1);
  const int64_t sps_max = ((1ll << 31) - 1) / (q2 * BK);
  return launch_gram8(ctx, d_zb, np_, kpad / BK, np_ * BK, q2, sps_max, true, d_gram, 0, (int)(np_ / BM3), np_);
}

int grid_knn_gram_kb_rows(grid_ctx *ctx, const uint16_t *d_zb, int64_t np_, int64_t kpad, int32_t qmax, int64_t row0,
                          int64_t nrows, int64_t *d_out, int64_t ld) {
  REQUIRE(ctx && d_zb && d_out, "bad args");
  REQUIRE(np_ > 0 && np_ % BM3 == 0, "np (%lld) must be a positive multiple of %d", (long long)np_, BM3);
  REQUIRE(kpad >= 0 && kpad % BK == 0, "kpad must be a multiple of %d", BK);
  REQUIRE(row0 >= 0 && nrows > 0 && row0 % BM3 == 0 && nrows % BM3 == 0 && row0 + nrows <= np_,
          "rows [%lld, %lld) must be whole 256-row tiles within np %lld", (long long)row0, (long long)(row0 + nrows),
          (long long)np_);
  REQUIRE(ld >= np_ - row0, "ld (%lld) below the segment width %lld", (long long)ld, (long long)(np_ - row0));
  REQUIRE(((uintptr_t)d_zb % 16) == 0 && ((uintptr_t)d_out % 8) == 0, "misaligned buffers");
  REQUIRE(qmax >= 0 && qmax <= 256, "qmax must be in [0, 256]");
  if (kpad == 0) return GRID_OK;
  const int64_t q2 = (int64_t)(qmax > 0 ? qmax : 1) * (qmax > 0 ? qmax : 1);
  const int64_t sps_max = ((1ll << 31) - 1) / (q2 * BK);
  // the kernel adds tile element (row, col) at base + row * ld + col: the
  // base sits row0 * (ld + 1) elements before d_out (never dereferenced there)
  int64_t *base = (int64_t *)((uintptr_t)d_out - (uintptr_t)(row0 * (ld + 1)) * sizeof(int64_t));
  return launch_gram8(ctx, d_zb, np_, kpad / BK, np_ * BK, q2, sps_max, true, base, (int)(row0 / BM3),
                      (int)((row0 + nrows) / BM3), ld);
}

int grid_knn_mirror(grid_ctx *ctx, int64_t *d_gram, int64_t np_) {
  REQUIRE(ctx && d_gram && np_ > 0 && np_ % 64 == 0, "np (%lld) must be a positive multiple of 64",
          (long long)np_);
  const int64_t nb = np_ / 64, pairs = nb * (nb - 1) / 2;
  if (pairs == 0) return GRID_OK;
  REQUIRE(pairs < (1ll << 31), "np too large");
  hipLaunchKernelGGL(k_mirror, dim3((unsigned)pairs), dim3(256), 0, ctx->stream, d_gram, np_);
  LAUNCHCHK();
  return GRID_OK;
}

int grid_knn_mirror_ld(grid_ctx *ctx, int64_t *d, int64_t n, int64_t ld) {
  REQUIRE(ctx && d && n >= 0 && n % 64 == 0 && ld >= n, "n (%lld) must be a multiple of 64 and <= ld",
          (long long)n);
  const int64_t nb = n / 64, pairs = nb * (nb - 1) / 2;
  if (pairs == 0) return GRID_OK;
  REQUIRE(pairs < (1ll << 31), "n too large");
  hipLaunchKernelGGL(k_mirror, dim3((unsigned)pairs), dim3(256), 0, ctx->stream, d, ld);
  LAUNCHCHK();
  return GRID_OK;
}

int grid_knn_diag(grid_ctx *ctx, const int64_t *d_gram, int64_t np_, int64_t n, int64_t *d_norms) {
  REQUIRE(ctx && d_gram && d_norms && n >= 0 && np_ >= n, "bad args");
  if (n == 0) return GRID_OK;
  hipLaunchKernelGGL(k_diag, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, ctx->stream, d_gram, np_, n, d_norms);
  LAUNCHCHK();
  return GRID_OK;
}

static int topk_checks(int64_t n, int64_t ld, int64_t k, int64_t row0, int64_t nrows) {
  REQUIRE(n > 0 && ld >= n && k >= 0, "bad args");
  REQUIRE(n <= (1 << 20), "n > 2^20 samples not supported by the packed key");
  REQUIRE(k + 1 <= SELCAP, "num_neighbors + 1 must be <= %d", SELCAP);
  REQUIRE(row0 >= 0 && nrows >= 0 && row0 + nrows <= n, "bad row block");
  REQUIRE(nrows < (1ll << 31), "too many rows");
  return GRID_OK;
}

int grid_knn_topk_rows(grid_ctx *ctx, const int64_t *d_rows, int64_t ld, const int64_t *d_norms, int64_t n,
                       int64_t k, int64_t row0, int64_t nrows, int32_t *d_idx, int64_t *d_d2, int32_t *d_cnt) {
  REQUIRE(ctx && d_rows && d_norms, "bad args");
  int rc = topk_checks(n, ld, k, row0, nrows);
  if (rc) return rc;
  if (nrows == 0 || k == 0) {
    if (nrows) HIPCHK(hipMemsetAsync(d_cnt, 0, nrows * 4, ctx->stream));
    return GRID_OK;
  }
  const int64_t ktake = k + 1 < n ? k + 1 : n;
  auto kern = ktake <= 16 ? k_topk_small<16, int64_t> : ktake <= 32 ? k_topk_small<32, int64_t>
                                                                      : k_topk_radix<int64_t>;
  hipLaunchKernelGGL(kern, dim3((unsigned)nrows), dim3(256), 0, ctx->stream, d_rows, ld, d_norms, 1.0, n, k, row0,
                     d_idx, (void *)d_d2, d_cnt, (int64_t)0, (unsigned long long *)nullptr);
  LAUNCHCHK();
  return GRID_OK;
}

int grid_knn_topk_d2(grid_ctx *ctx, const double *d_d2rows, int64_t ld, double key_scale, int64_t n, int64_t k,
                     int64_t row0, int64_t nrows, int32_t *d_idx, double *d_d2, int32_t *d_cnt) {
  REQUIRE(ctx && d_d2rows && key_scale > 0.0, "bad args");
  int rc = topk_checks(n, ld, k, row0, nrows);
  if (rc) return rc;
  if (nrows == 0 || k == 0) {
    if (nrows) HIPCHK(hipMemsetAsync(d_cnt, 0, nrows * 4, ctx->stream));
    return GRID_OK;
  }
  hipLaunchKernelGGL(k_topk_d2, dim3((unsigned)nrows), dim3(256), 0, ctx->stream, d_d2rows, ld, n, k, row0, d_idx,
                     d_d2, d_cnt);
  LAUNCHCHK();
  return GRID_OK;
}

int grid_knn_panel_i32(grid_ctx *ctx, const int32_t *d_zq, int64_t n, int64_t ld, const int32_t *d_cols, int64_t r,
                       int32_t qmax, uint16_t *d_zb, int64_t np_, int64_t kpad) {
  REQUIRE(ctx && d_zq && d_zb && n >= 0 && r >= 0 && (r == 0 || d_cols), "bad args");
  REQUIRE(np_ >= n && np_ % 64 == 0 && np_ <= 65535 && kpad >= r && kpad % 64 == 0, "bad panel shape");
  REQUIRE(qmax >= 0 && qmax <= 256, "qmax must be in [0, 256] (bf16-exact)");
  if (kpad == 0) return GRID_OK;
  hipLaunchKernelGGL(k_panel_i32, dim3((unsigned)ceil_div(kpad, 256), (unsigned)np_), dim3(256), 0, ctx->stream,
                     d_zq, n, ld, d_cols, r, qmax, d_zb, np_, kpad);
  LAUNCHCHK();
  return GRID_OK;
}

int grid_knn_gather_i32(grid_ctx *ctx, const int32_t *d_zq, int64_t n, int64_t ld, const int32_t *d_cols, int64_t r,
                        int32_t qmax, int32_t *d_out) {
  REQUIRE(ctx && d_zq && d_out && n >= 0 && n <= 65535 && r >= 0 && (r == 0 || d_cols) && qmax >= 0, "bad args");
  if (n == 0 || r == 0) return GRID_OK;
  hipLaunchKernelGGL(k_gather_i32, dim3((unsigned)ceil_div(r, 256), (unsigned)n), dim3(256), 0, ctx->stream, d_zq, n,
                     ld, d_cols, r, qmax, d_out);
  LAUNCHCHK();
  return GRID_OK;
}

int grid_knn_gather_f64(grid_ctx *ctx, const int32_t *d_zq, int64_t n, int64_t ld, const int32_t *d_cols, int64_t r,
                        double zmax, double *d_out) {
  REQUIRE(ctx && d_zq && d_out && n >= 0 && n <= 65535 && r >= 0 && (r == 0 || d_cols), "bad args");
  if (n == 0 || r == 0) return GRID_OK;
  hipLaunchKernelGGL(k_gather_f64, dim3((unsigned)ceil_div(r, 256), (unsigned)n), dim3(256), 0, ctx->stream, d_zq, n,
                     ld, d_cols, r, zmax, d_out);
  LAUNCHCHK();
  return GRID_OK;
}

static int dist_launch(grid_ctx *ctx, const void *d_z, bool is_int, int64_t n, int64_t r, int64_t ld, double *d_d2,
                       int64_t np_) {
  REQUIRE(ctx && d_z && d_d2 && n >= 0 && r >= 0 && ld >= r && np_ >= n && np_ % 64 == 0, "bad args");
  const int64_t nb = np_ / 64, tiles = nb * (nb + 1) / 2;
  if (tiles == 0) return GRID_OK;
  REQUIRE(tiles < (1ll << 31), "np too large");
  if (is_int)
    hipLaunchKernelGGL((k_dist<int32_t, int64_t>), dim3((unsigned)tiles), dim3(256), 0, ctx->stream,
                       (const int32_t *)d_z, ld, n, r, d_d2, np_, nb);
  else
    hipLaunchKernelGGL((k_dist<double, double>), dim3((unsigned)tiles), dim3(256), 0, ctx->stream,
                       (const double *)d_z, ld, n, r, d_d2, np_, nb);
  LAUNCHCHK();
  return grid_knn_mirror(ctx, (int64_t *)d_d2, np_);
}

int grid_knn_dist_i32(grid_ctx *ctx, const int32_t *d_z, int64_t n, int64_t r, int64_t ld, double *d_d2,
                      int64_t np_) {
  return dist_launch(ctx, d_z, true, n, r, ld, d_d2, np_);
}

int grid_knn_dist_f64(grid_ctx *ctx, const double *d_z, int64_t n, int64_t r, int64_t ld, double *d_d2,
                      int64_t np_) {
  return dist_launch(ctx, d_z, false, n, r, ld, d_d2, np_);
}

int grid_knn_topk(grid_ctx *ctx, int64_t *d_gram, int64_t n, int64_t np_, int64_t k, int64_t row0,
                  int64_t nrows, int32_t *d_idx, int64_t *d_d2, int32_t *d_cnt) {
  REQUIRE(ctx && d_gram && n > 0 && np_ >= n && np_ % 64 == 0 && k >= 0, "bad args");
  int rc = grid_knn_mirror(ctx, d_gram, np_);
  if (rc) return rc;
  void *s = nullptr;
  rc = grid_scratch(ctx, (size_t)n * 8, &s);
  if (rc) return rc;
  int64_t *nrm = (int64_t *)s;
  rc = grid_knn_diag(ctx, d_gram, np_, n, nrm);
  if (rc) return rc;
  return grid_knn_topk_rows(ctx, d_gram + row0 * np_, np_, nrm, n, k, row0, nrows, d_idx, d_d2, d_cnt);
}

int grid_knn_seg_topk(grid_ctx *ctx, const int64_t *d_seg, int64_t ld, int64_t nrows, int64_t ncols,
                      const int64_t *d_norms, int64_t n, int64_t k, int64_t r0, int64_t c0,
                      unsigned long long *d_rowc, unsigned long long *d_colc) {
  REQUIRE(ctx && d_seg && d_norms && d_rowc && d_colc, "bad args");
  REQUIRE(n > 0 && n <= (1 << 20) && k >= 0 && k + 1 <= GRID_SEG_K1, "bad n / k (k + 1 <= %d)", GRID_SEG_K1);
  REQUIRE(nrows >= 0 && ncols >= 0 && ld >= ncols && r0 >= 0 && c0 >= 0, "bad segment");
  // rows of the segment that are samples: row lists (raw mode, columns [c0, n))
  const int64_t rr = r0 < n ? (n - r0 < nrows ? n - r0 : nrows) : 0;
  if (rr > 0) {
    hipLaunchKernelGGL((k_topk_small<GRID_SEG_K1, int64_t>), dim3((unsigned)rr), dim3(256), 0, ctx->stream,
                       d_seg - c0, ld, d_norms, 1.0, n, k, r0, (int32_t *)nullptr, (void *)nullptr,
                       (int32_t *)nullptr, c0, d_rowc);
    LAUNCHCHK();
  }
  if (nrows > rr) {          // padding rows: no candidates
    HIPCHK(hipMemsetAsync(d_rowc + rr * GRID_SEG_K1, 0xFF, (nrows - rr) * GRID_SEG_K1 * 8, ctx->stream));
  }
  if (ncols > 0) {
    hipLaunchKernelGGL(k_seg_cols<GRID_SEG_K1>, dim3((unsigned)((ncols + 31) / 32)), dim3(256), 0, ctx->stream,
                       d_seg, ld, nrows, ncols, d_norms, n, r0, c0, d_colc);
    LAUNCHCHK();
  }
  return GRID_OK;
}

int grid_knn_seg_merge(grid_ctx *ctx, const unsigned long long *d_rowc, const unsigned long long *d_colc,
                       int64_t ldc, int64_t B, int64_t n, int64_t k, int32_t *d_idx, int64_t *d_d2,
                       int32_t *d_cnt) {
  REQUIRE(ctx && d_rowc && d_colc && d_idx && d_d2 && d_cnt, "bad args");
  REQUIRE(n > 0 && n <= (1 << 20) && k >= 0 && k + 1 <= GRID_SEG_K1 && B > 0 && ldc >= B, "bad args");
  if (k == 0) {
    HIPCHK(hipMemsetAsync(d_cnt, 0, n * 4, ctx->stream));
    return GRID_OK;
  }
  // the wave-per-row form while a row's candidates fit 8 keys per lane (2W + 1
  // lists of K1: W <= 15 at K1 = 16), the thread-per-row form beyond
  const int64_t blocks = (n + B - 1) / B;
  if (GRID_SEG_K1 * (blocks + 1) <= 64 * 8) {
    hipLaunchKernelGGL((k_seg_merge_w<GRID_SEG_K1, 8>), dim3((unsigned)((n + 3) / 4)), dim3(256), 0, ctx->stream,
                       d_rowc, d_colc, ldc, B, n, k, d_idx, d_d2, d_cnt);
  } else {
    hipLaunchKernelGGL(k_seg_merge<GRID_SEG_K1>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, d_rowc,
                       d_colc, ldc, B, n, k, d_idx, d_d2, d_cnt);
  }
  LAUNCHCHK();
  return GRID_OK;
}

int grid_knn_seg_pack(grid_ctx *ctx, const int64_t *d_gram, int64_t np_, int64_t W, int64_t B, int64_t *d_send) {
  REQUIRE(ctx && d_gram && d_send && np_ > 0 && W > 0 && B > 0 && 2 * W * B >= np_ && W <= 32768 && B <= (1 << 30),
          "bad args");
  hipLaunchKernelGGL(k_seg_pack, dim3((unsigned)B, (unsigned)(2 * W)), dim3(256), 0, ctx->stream, d_gram, np_, W, B,
                     d_send);
  LAUNCHCHK();
  return GRID_OK;
}

int grid_knn_seg_tiles_pack(grid_ctx *ctx, const int64_t *d_seg, int64_t ld, int64_t B, int64_t W, int64_t b_src,
                            int64_t *d_send) {
  REQUIRE(ctx && d_seg && d_send, "bad args");
  REQUIRE(W > 0 && W <= 32768 && B > 0 && B <= (1 << 20), "bad W / B (W <= 32768, B <= 2^20)");
  REQUIRE(b_src >= 0 && b_src < 2 * W, "block %lld outside [0, 2W)", (long long)b_src);
  REQUIRE(ld >= (2 * W - b_src) * B, "ld (%lld) below the segment width %lld", (long long)ld,
          (long long)((2 * W - b_src) * B));
  const int64_t tiles = 2 * W - 1 - b_src, sub = ceil_div(B, 32);
  if (tiles == 0) return GRID_OK;            // the last block sends nothing
  hipLaunchKernelGGL(k_seg_tiles_pack, dim3((unsigned)sub, (unsigned)sub, (unsigned)tiles), dim3(256), 0, ctx->stream,
                     d_seg, ld, B, W, b_src, d_send);
  LAUNCHCHK();
  return GRID_OK;
}

int grid_knn_seg_rows_fill(grid_ctx *ctx, const int64_t *d_seg, int64_t ld, const int64_t *d_recv, int64_t B,
                           int64_t W, int64_t b, int64_t *d_rows, int64_t ld_rows) {
  REQUIRE(ctx && d_seg && d_recv && d_rows, "bad args");
  REQUIRE(W > 0 && W <= 32768 && B > 0 && B <= (1 << 20), "bad W / B (W <= 32768, B <= 2^20)");
  REQUIRE(b >= 0 && b < 2 * W, "block %lld outside [0, 2W)", (long long)b);
  REQUIRE(ld >= (2 * W - b) * B, "ld (%lld) below the segment width %lld", (long long)ld,
          (long long)((2 * W - b) * B));
  REQUIRE(ld_rows >= 2 * W * B, "ld_rows (%lld) below the row width %lld", (long long)ld_rows,
          (long long)(2 * W * B));
  hipLaunchKernelGGL(k_seg_rows_fill, dim3((unsigned)B, (unsigned)(2 * W)), dim3(256), 0, ctx->stream, d_seg, ld,
                     d_recv, B, W, b, d_rows, ld_rows);
  LAUNCHCHK();
  return GRID_OK;
}

}  // extern "C"
