// The normalised-matrix row text (textio.cpp: "ID \t scale \t z_1 ... z_R \n")
// as the device reader parses it, compiled for host and device: the kernels
// of ntext_dev.hip and their serial host restatement (grid_ntext_parse_host)
// run the functions below, so the CPU tests check the grammar and the field
// arithmetic the GPU runs.
//
// A member's text is cut in CH-byte chunks and SEG-byte segments.  A FIELD is
// the bytes between two separators (tab or newline); its ordinal f is the
// number of separators before it in the member.  With F = R + 2 fields per
// row, field f belongs to row first_row + f / F and is the ID (f % F == 0),
// the scale (1) or cell f % F - 2; the separator ending it must be a newline
// exactly when f % F == F - 1.  A field is handled by the segment that holds
// its first byte.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define NT_HD __host__ __device__ __forceinline__
#else
#define NT_HD inline
#endif

namespace ntext {

constexpr int CH = 16384, SEG = 64;
constexpr int MAXCELL = 12;          // "-21474836.47"
constexpr int LOOK = 16;             // bytes after a chunk its last field may need (MAXCELL + its separator)
constexpr int32_t MISSING = (int32_t)0x80000000;   // GRID_MISSING

// per-member flag bits (include/grid_abi.h GRID_NT_*)
constexpr int BADCELL = 1, BADROW = 2, LEADWS = 4, CR = 8, NOEOL = 16, ROWRANGE = 32, PREFIX = 64;

// One cell [p, p + len): what textio.cpp parse_hundredths accepts, with the
// same value -- "NA" / "nan", or -?D{1,8}.DD with magnitude <= 2147483647
// ("-0.00" -> 0).  Nine or more integer digits, which that parser takes while
// leading zeros keep the value in range, are refused here (the host reader
// then reads the file).
template <class P>
NT_HD bool cell(const P &p, int len, int32_t &v) {
  if ((len == 2 && p[0] == 'N' && p[1] == 'A') || (len == 3 && p[0] == 'n' && p[1] == 'a' && p[2] == 'n')) {
    v = MISSING;
    return true;
  }
  int i = 0;
  const bool neg = len > 0 && p[0] == '-';
  i += neg;
  const int nd = len - 3 - i;        // integer digits
  if (nd < 1 || nd > 8 || p[len - 3] != '.') return false;
  int64_t a = 0;
  for (int k = 0; k < nd; k++) {
    const unsigned d = (unsigned)p[i + k] - '0';
    if (d > 9) return false;
    a = a * 10 + d;
  }
  const unsigned f0 = (unsigned)p[len - 2] - '0', f1 = (unsigned)p[len - 1] - '0';
  if (f0 > 9 || f1 > 9) return false;
  a = a * 100 + f0 * 10 + f1;
  if (a > 2147483647ll) return false;
  v = (int32_t)(neg ? -a : a);
  return true;
}

NT_HD bool is_sep(uint8_t c) { return c == '\t' || c == '\n'; }

template <class T>
struct Sub {                         // the member's bytes from x on
  const T &t;
  int64_t x;
  NT_HD uint8_t operator[](int k) const { return t[x + k]; }
};

struct Out {
  int32_t *zq;        // [n][ld]
  int64_t ld, n, r;
  int64_t *rowoff;    // [n]: byte offset of the row's text (tbase + its offset in the member)
};

// The fields that start in segment [s0, s1) of a member of L bytes, and the
// separators inside it.  t[x]: byte x of the member, readable for
// max(0, s0 - 1) <= x < min(L, s1 + LOOK).  sep: bit j = byte s0 + j is a
// separator.  f0: separators in [0, s0).  Returns flag bits.
template <class T>
NT_HD int segment(const T &t, uint64_t sep, int64_t s0, int64_t s1, int64_t L, int64_t f0, int64_t first_row,
                  int64_t tbase, const Out &o) {
  const int64_t F = o.r + 2;
  int64_t row = first_row + f0 / F;
  int64_t k = f0 % F;                // position of field f in its row
  int bad = 0;
  auto field = [&](int64_t x, int len) {   // len < 0: no separator within MAXCELL + 1 bytes
    if (k == 0) {
      if (row < 0 || row >= o.n) bad |= ROWRANGE;
      else o.rowoff[row] = tbase + x;
      if (t[x] == ' ' || t[x] == '\t') bad |= LEADWS;
    } else if (k >= 2) {
      int32_t v;
      if (len < 0 || len > MAXCELL || !cell(Sub<T>{t, x}, len, v)) bad |= BADCELL;
      else if (row >= 0 && row < o.n) o.zq[row * o.ld + (k - 2)] = v;
    }
  };
  int64_t cur = (s0 == 0 || is_sep(t[s0 - 1])) ? s0 : -1;
  while (sep) {
    const int j = __builtin_ctzll(sep);
    sep &= sep - 1;
    const int64_t y = s0 + j;
    if (cur >= 0) field(cur, (int)(y - cur));
    if ((t[y] == '\n') != (k == F - 1)) bad |= BADROW;
    if (++k == F) { k = 0; row++; }
    cur = y + 1 < s1 ? y + 1 : -1;
  }
  if (cur >= 0) {                    // starts here, ends in a later segment
    int len = -1;
    if (k >= 2) {
      const int64_t lim = (L - cur < MAXCELL + 1 ? L - cur : MAXCELL + 1);
      for (int e = (int)(s1 - cur); e < lim; e++)
        if (is_sep(t[cur + e])) { len = e; break; }
    }
    field(cur, len);
  }
  if (s1 == L && s1 > s0 && t[L - 1] != '\n') bad |= NOEOL;
  return bad;
}

}  // namespace ntext
