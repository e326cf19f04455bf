// Step-5 read on the device: the normalised-matrix text (textio.cpp's file,
// its row members inflated in HBM by inflate.hip) -> the int32 hundredths
// matrix zq [N][R].  The mirror of gzwrite.hip, in the pattern of
// mosdepth_dev.hip.  A batch is the text of several row members laid end to
// end (member m: d_text + toff[m], tlen[m] bytes, rows from first_row[m]);
// every member is cut in 16 KiB chunks.
//
// Kernels per batch: k_nt_count (separators and newlines per chunk, any
// '\r'), k_nt_scan (per member: the field ordinal at each chunk start, the
// member's rows), k_nt_parse (one workgroup per chunk: the chunk and a
// look-ahead of one maximal cell in LDS, one thread per 64-byte segment,
// each field parsed by the thread whose segment holds its first byte:
// ntext_core.hpp), k_nt_prefix (the first GRID_NT_PREFIX bytes of every row,
// from which the host takes the ID and the scale with its own parse_float).
// Anything outside the writer's grammar sets a per-member flag and never a
// value the host reader would not give; the caller then reads the file with
// the host reader.
#include "common.hpp"
#include "ntext_core.hpp"

#include <vector>

namespace {

using ntext::CH;
using ntext::LOOK;
using ntext::SEG;
constexpr int PTH = CH / SEG, HALO = 16;
constexpr int SPAN = HALO + CH + LOOK;          // bytes a - 16 .. b + LOOK of the member
static_assert(GRID_NT_BADCELL == ntext::BADCELL && GRID_NT_BADROW == ntext::BADROW &&
                  GRID_NT_LEADWS == ntext::LEADWS && GRID_NT_CR == ntext::CR && GRID_NT_NOEOL == ntext::NOEOL &&
                  GRID_NT_ROWRANGE == ntext::ROWRANGE && GRID_NT_PREFIX == ntext::PREFIX &&
                  GRID_MISSING == ntext::MISSING,
              "include/grid_abi.h and ntext_core.hpp disagree");

// bit 7 of every byte of w equal to c (exact per byte)
__host__ __device__ __forceinline__ uint32_t eq_bytes(uint32_t w, uint32_t c) {
  const uint32_t x = w ^ (c * 0x01010101u);
  return ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu);
}

// separators (tab or newline) and newlines per chunk; any '\r' -> GRID_NT_CR
__global__ __launch_bounds__(256) void k_nt_count(const uint8_t *__restrict__ text, const int64_t *__restrict__ toff,
                                                  const int64_t *__restrict__ tlen, const int32_t *__restrict__ cfile,
                                                  const int64_t *__restrict__ cstart, int32_t *__restrict__ csep,
                                                  int32_t *__restrict__ cnl, int32_t *__restrict__ flags,
                                                  const int32_t *__restrict__ mst) {
  const int c = blockIdx.x, m = cfile[c];
  if (mst && mst[m]) return;            // a member that did not inflate: its text is never read
  const int64_t a = cstart[c], b = min(tlen[m], a + CH);
  const uint8_t *t = text + toff[m];
  int ns = 0, nn = 0, cr = 0;
  for (int64_t i = a + threadIdx.x * 16; i < b; i += 256 * 16) {
    if (i + 16 <= b) {
      const uint4 v = *reinterpret_cast<const uint4 *>(t + i);
      const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const uint32_t n = eq_bytes(w[k], '\n');
        nn += __builtin_popcount(n);
        ns += __builtin_popcount(n | eq_bytes(w[k], '\t'));
        cr |= eq_bytes(w[k], '\r') != 0;
      }
    } else {
      for (int64_t j = i; j < b; j++) {
        nn += t[j] == '\n';
        ns += t[j] == '\n' || t[j] == '\t';
        cr |= t[j] == '\r';
      }
    }
  }
  for (int o = 32; o > 0; o >>= 1) {
    ns += __shfl_xor(ns, o, 64);
    nn += __shfl_xor(nn, o, 64);
    cr |= __shfl_xor(cr, o, 64);
  }
  __shared__ int s_s[4], s_n[4], s_c[4];
  if ((threadIdx.x & 63) == 0) {
    s_s[threadIdx.x >> 6] = ns;
    s_n[threadIdx.x >> 6] = nn;
    s_c[threadIdx.x >> 6] = cr;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    csep[c] = s_s[0] + s_s[1] + s_s[2] + s_s[3];
    cnl[c] = s_n[0] + s_n[1] + s_n[2] + s_n[3];
    if (s_c[0] | s_c[1] | s_c[2] | s_c[3]) atomicOr(flags + m, GRID_NT_CR);
  }
}

// per member: separators before each chunk (exclusive prefix over its
// chunks) and its newlines.  A workgroup per member, 256 chunks per round.
__global__ __launch_bounds__(256) void k_nt_scan(const int32_t *__restrict__ cfirst, const int32_t *__restrict__ csep,
                                                 const int32_t *__restrict__ cnl, int64_t *__restrict__ cfield0,
                                                 int64_t *__restrict__ nrows, int nmem,
                                                 const int32_t *__restrict__ mst) {
  __shared__ int64_t s_w[4], s_r[4];
  const int m = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  if (m >= nmem) return;
  if (mst && mst[m]) {
    if (tid == 0) nrows[m] = 0;
    return;
  }
  const int c0 = cfirst[m], c1 = cfirst[m + 1];
  int64_t base = 0, rows = 0;
  for (int r = c0; r < c1; r += 256) {
    const int c = r + tid;
    const int64_t v = c < c1 ? csep[c] : 0;
    int64_t incl = v, nl = c < c1 ? cnl[c] : 0;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int64_t y = __shfl_up(incl, d, 64);
      if (lane >= d) incl += y;
    }
    for (int o = 32; o > 0; o >>= 1) nl += __shfl_xor(nl, o, 64);
    if (lane == 63) s_w[wv] = incl;
    if (lane == 0) s_r[wv] = nl;
    __syncthreads();
    int64_t before = base;
    for (int w = 0; w < wv; w++) before += s_w[w];
    if (c < c1) cfield0[c] = before + incl - v;
    base += s_w[0] + s_w[1] + s_w[2] + s_w[3];
    rows += s_r[0] + s_r[1] + s_r[2] + s_r[3];
    __syncthreads();
  }
  if (tid == 0) nrows[m] = rows;
}

// The chunk in LDS with 4 bytes of padding after every 64-byte block, as
// mosdepth_dev.hip lays it out (block t + 1 holds segment t, the 16-byte
// halo sits in block 0): the 64 lanes of a wave reading "their" byte k hit
// 64 different banks.
__device__ __forceinline__ int nt_phys(int i) { return i + 4 * ((i + 48) >> 6); }
struct LdsText {
  const uint8_t *s;
  int64_t a;                            // member offset of the chunk's first byte
  __device__ __forceinline__ uint8_t operator[](int64_t x) const { return s[nt_phys(HALO + (int)(x - a))]; }
};

__global__ __launch_bounds__(PTH) void k_nt_parse(const uint8_t *__restrict__ text, const int64_t *__restrict__ toff,
                                                  const int64_t *__restrict__ tlen,
                                                  const int64_t *__restrict__ first_row,
                                                  const int32_t *__restrict__ cfile,
                                                  const int64_t *__restrict__ cstart,
                                                  const int64_t *__restrict__ cfield0, ntext::Out o,
                                                  int32_t *__restrict__ flags, const int32_t *__restrict__ mst) {
  static_assert(HALO == 16 && SEG == 64, "nt_phys: block t + 1 = segment t");
  __shared__ __attribute__((aligned(16))) uint8_t s_t[SPAN + 16 + 4 * ((SPAN + 16) / 64 + 2)];
  __shared__ int s_wsum[PTH / 64];
  const int c = blockIdx.x, m = cfile[c], tid = threadIdx.x;
  if (mst && mst[m]) return;
  const int64_t L = tlen[m], a = cstart[c], b = min(L, a + CH);
  const uint8_t *t = text + toff[m];
  // load [a - 16, min(L, b + LOOK)): whole 16-byte words inside the member
  // (text offsets are 256-B aligned, chunk starts multiples of CH), the last
  // partial word byte by byte, zeros past the end
  {
    const int64_t lo = a - HALO, hi = min(L, b + LOOK);
    constexpr int NW = (SPAN + 15) / 16, G = 3;
    for (int k0 = 0; k0 * PTH < NW; k0 += G) {
      uint4 v[G];
#pragma unroll
      for (int k = 0; k < G; k++) {
        const int w = tid + (k0 + k) * PTH;
        const int64_t p = lo + 16 * (int64_t)w;
        v[k] = make_uint4(0, 0, 0, 0);
        if (w < NW && p >= 0 && p + 16 <= hi) v[k] = *reinterpret_cast<const uint4 *>(t + p);
      }
#pragma unroll
      for (int k = 0; k < G; k++) {
        const int w = tid + (k0 + k) * PTH;
        const int64_t p = lo + 16 * (int64_t)w;
        if (w >= NW) continue;
        if (p >= 0 && p + 16 > hi && p < hi) {
          uint8_t q[16];
          for (int j = 0; j < 16; j++) q[j] = p + j < hi ? t[p + j] : 0;
          v[k] = *reinterpret_cast<const uint4 *>(q);
        }
        uint32_t *d = reinterpret_cast<uint32_t *>(s_t + nt_phys(16 * w));
        d[0] = v[k].x;
        d[1] = v[k].y;
        d[2] = v[k].z;
        d[3] = v[k].w;
      }
    }
  }
  __syncthreads();
  // my segment [s0, s1): its separator mask and count
  const int64_t s0 = a + (int64_t)tid * SEG, s1 = min(b, s0 + SEG);
  uint64_t sep = 0;
  if (s1 > s0) {
    const uint32_t *seg = reinterpret_cast<const uint32_t *>(s_t + nt_phys(HALO + tid * SEG));
#pragma unroll
    for (int k = 0; k < SEG / 4; k++) {
      const uint32_t z = eq_bytes(seg[k], '\t') | eq_bytes(seg[k], '\n');
      const uint64_t four = ((z >> 7) & 1u) | ((z >> 14) & 2u) | ((z >> 21) & 4u) | ((z >> 28) & 8u);
      sep |= four << (4 * k);
    }
    if (s1 - s0 < SEG) sep &= (1ull << (s1 - s0)) - 1ull;
  }
  const int ns = __builtin_popcountll(sep);
  int incl = ns;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int y = __shfl_up(incl, d, 64);
    if ((tid & 63) >= d) incl += y;
  }
  if ((tid & 63) == 63) s_wsum[tid >> 6] = incl;
  __syncthreads();
  int before = incl - ns;
  for (int w = 0; w < (tid >> 6); w++) before += s_wsum[w];
  if (s1 > s0) {
    const int bad = ntext::segment(LdsText{s_t, a}, sep, s0, s1, L, cfield0[c] + before, first_row[m], toff[m], o);
    if (bad) atomicOr(flags + m, bad);
  }
}

// the first GRID_NT_PREFIX bytes of every row this batch placed (rowoff >= 0,
// reset to -1 for the next batch), zero filled past the batch's text
__global__ __launch_bounds__(64) void k_nt_prefix(const uint8_t *__restrict__ text, int64_t text_end,
                                                  int64_t *__restrict__ rowoff, int64_t n,
                                                  uint8_t *__restrict__ pre) {
  const int64_t row = blockIdx.x;
  if (row >= n) return;
  const int64_t off = rowoff[row];
  if (off < 0) return;
  for (int j = threadIdx.x; j < GRID_NT_PREFIX_BYTES; j += 64)
    pre[row * GRID_NT_PREFIX_BYTES + j] = off + j < text_end ? text[off + j] : 0;
  __syncthreads();
  if (threadIdx.x == 0) rowoff[row] = -1;
}

struct HostText {
  const uint8_t *p;
  uint8_t operator[](int64_t x) const { return p[x]; }
};

}  // namespace

extern "C" {

int grid_ntext_count(grid_ctx *ctx, const uint8_t *d_text, const int64_t *d_toff, const int64_t *d_tlen,
                     int64_t nchunks, const int32_t *d_cfile, const int64_t *d_cstart, const int32_t *d_cfirst,
                     int64_t nmembers, int32_t *d_csep, int32_t *d_cnl, int64_t *d_cfield0, int64_t *d_nrows,
                     int32_t *d_flags, const int32_t *d_mstatus) {
  REQUIRE(ctx && nchunks >= 0 && nchunks <= 0x7fffffff && nmembers >= 0 && nmembers <= 0x7fffffff, "bad args");
  if (nmembers == 0) return GRID_OK;
  REQUIRE(d_toff && d_tlen && d_cfirst && d_nrows && d_flags, "null pointer");
  if (nchunks > 0) {
    REQUIRE(d_text && d_cfile && d_cstart && d_csep && d_cnl && d_cfield0, "null pointer");
    hipLaunchKernelGGL(k_nt_count, dim3((unsigned)nchunks), dim3(256), 0, ctx->stream, d_text, d_toff, d_tlen,
                       d_cfile, d_cstart, d_csep, d_cnl, d_flags, d_mstatus);
    LAUNCHCHK();
  }
  hipLaunchKernelGGL(k_nt_scan, dim3((unsigned)nmembers), dim3(256), 0, ctx->stream, d_cfirst, d_csep, d_cnl,
                     d_cfield0, d_nrows, (int)nmembers, d_mstatus);
  LAUNCHCHK();
  return GRID_OK;
}

int grid_ntext_parse(grid_ctx *ctx, const uint8_t *d_text, const int64_t *d_toff, const int64_t *d_tlen,
                     const int64_t *d_first_row, int64_t nchunks, const int32_t *d_cfile, const int64_t *d_cstart,
                     const int64_t *d_cfield0, int64_t n, int64_t r, int32_t *d_zq, int64_t ld, int64_t *d_rowoff,
                     int32_t *d_flags, const int32_t *d_mstatus) {
  REQUIRE(ctx && nchunks >= 0 && nchunks <= 0x7fffffff && n > 0 && r > 0 && ld >= r, "bad args");
  if (nchunks == 0) return GRID_OK;
  REQUIRE(d_text && d_toff && d_tlen && d_first_row && d_cfile && d_cstart && d_cfield0 && d_zq && d_rowoff &&
              d_flags, "null pointer");
  const ntext::Out o{d_zq, ld, n, r, d_rowoff};
  hipLaunchKernelGGL(k_nt_parse, dim3((unsigned)nchunks), dim3(PTH), 0, ctx->stream, d_text, d_toff, d_tlen,
                     d_first_row, d_cfile, d_cstart, d_cfield0, o, d_flags, d_mstatus);
  LAUNCHCHK();
  return GRID_OK;
}

int grid_ntext_prefix(grid_ctx *ctx, const uint8_t *d_text, int64_t text_bytes, int64_t *d_rowoff, int64_t n,
                      uint8_t *d_prefix) {
  REQUIRE(ctx && n >= 0 && n <= 0x7fffffff && text_bytes >= 0, "bad args");
  if (n == 0) return GRID_OK;
  REQUIRE(d_text && d_rowoff && d_prefix, "null pointer");
  hipLaunchKernelGGL(k_nt_prefix, dim3((unsigned)n), dim3(64), 0, ctx->stream, d_text, text_bytes, d_rowoff, n,
                     d_prefix);
  LAUNCHCHK();
  return GRID_OK;
}

// The kernels' count / scan / parse over one member's text in host memory,
// chunk by chunk and segment by segment (no GPU): the same ntext_core.hpp.
int grid_ntext_parse_host(const uint8_t *h_text, int64_t len, int64_t first_row, int64_t n, int64_t r, int32_t *h_zq,
                          int64_t ld, int64_t *h_rowoff, int64_t tbase, int32_t *flags, int64_t *nrows) {
  REQUIRE(len >= 0 && (len == 0 || h_text) && n > 0 && r > 0 && ld >= r && h_zq && h_rowoff && flags && nrows,
          "bad args");
  const int64_t nch = (len + CH - 1) / CH;
  // count
  std::vector<int64_t> csep((size_t)nch + 1, 0), cfield0((size_t)nch + 1, 0);
  int bad = 0;
  int64_t rows = 0;
  for (int64_t c = 0; c < nch; c++)
    for (int64_t i = c * CH; i < std::min(len, (c + 1) * CH); i++) {
      csep[c] += ntext::is_sep(h_text[i]);
      rows += h_text[i] == '\n';
      if (h_text[i] == '\r') bad |= GRID_NT_CR;
    }
  // scan
  for (int64_t c = 0; c < nch; c++) cfield0[c + 1] = cfield0[c] + csep[c];
  // parse
  const ntext::Out o{h_zq, ld, n, r, h_rowoff};
  const HostText t{h_text};
  for (int64_t c = 0; c < nch; c++) {
    const int64_t a = c * CH, b = std::min(len, a + CH);
    int64_t before = 0;
    for (int tid = 0; tid < PTH; tid++) {
      const int64_t s0 = a + (int64_t)tid * SEG, s1 = std::min(b, s0 + SEG);
      if (s1 <= s0) break;
      uint64_t sep = 0;
      for (int64_t j = s0; j < s1; j++)
        if (ntext::is_sep(h_text[j])) sep |= 1ull << (j - s0);
      bad |= ntext::segment(t, sep, s0, s1, len, cfield0[c] + before, first_row, tbase, o);
      before += __builtin_popcountll(sep);
    }
  }
  *flags = bad;
  *nrows = rows;
  return GRID_OK;
}

}  // extern "C"
