// Synthetic mosdepth cohort on disk for the from-files end-to-end run
// (tools/e2e_files.py): one DIR/S%05d.regions.bed.gz per sample, lines
// "chr1\tSTART\tEND\tDEPTH\n" with 1 kb bins and DEPTH printed "%.2f" like
// mosdepth.  The depth model is the bench cohort's (grid_amd/csrc/
// synth_model.hpp, restated for the host: per-bin base and cluster offset,
// one 64-bit hash per cell).  Samples are written in parallel, gzip level 1:
// one gzip member per file, or with "bgzf" BGZF (what mosdepth writes through
// htslib: 65280-byte blocks, each its own member with the "BC" length field,
// then the 28-byte end-of-file member).
//   g++ -O3 -std=c++17 -pthread -o tools/gen_cohort tools/gen_cohort.cpp -lz -ldl
//   tools/gen_cohort DIR N_SAMPLES N_BINS SEED THREADS [FIRST_SAMPLE [bgzf]]
// (samples FIRST_SAMPLE .. FIRST_SAMPLE + N_SAMPLES - 1: batches of one cohort)
#include <dlfcn.h>
#include <zlib.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

static inline uint64_t mix(uint64_t z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
static inline float unif(uint64_t h) { return (float)(h >> 40) * (1.0f / 16777216.0f); }
// libdeflate (the system library, loaded at run time; its header is not in the
// image) for the BGZF blocks: ~3x zlib's level-1 rate; zlib without it
struct Ldf {
  void *(*alloc_c)(int) = nullptr;
  size_t (*deflate_c)(void *, const void *, size_t, void *, size_t) = nullptr;
  void (*free_c)(void *) = nullptr;
  uint32_t (*crc)(uint32_t, const void *, size_t) = nullptr;
  bool ok = false;
  Ldf() {
    if (getenv("GRID_NO_LIBDEFLATE")) return;
    void *h = dlopen("libdeflate.so.0", RTLD_NOW | RTLD_LOCAL);
    if (!h) return;
    alloc_c = (void *(*)(int))dlsym(h, "libdeflate_alloc_compressor");
    deflate_c = (size_t (*)(void *, const void *, size_t, void *, size_t))dlsym(h, "libdeflate_deflate_compress");
    free_c = (void (*)(void *))dlsym(h, "libdeflate_free_compressor");
    crc = (uint32_t (*)(uint32_t, const void *, size_t))dlsym(h, "libdeflate_crc32");
    ok = alloc_c && deflate_c && free_c && crc;
  }
};
static const Ldf g_ldf;
// BGZF writer: text in, 65280-byte blocks out as gzip members
struct Bgzf {
  FILE *f = nullptr;
  std::vector<char> blk;
  std::vector<unsigned char> z;
  void *comp = nullptr;           // libdeflate compressor (level 1), one per writer
  bool ok = true;
  explicit Bgzf(FILE *ff) : f(ff), z(70000) {
    blk.reserve(65280);
    if (g_ldf.ok) comp = g_ldf.alloc_c(1);
  }
  ~Bgzf() {
    if (comp) g_ldf.free_c(comp);
  }
  void block(const char *p, size_t n, int level) {
    size_t c = 0;
    int rc = Z_STREAM_END;
    if (comp && level) {
      c = g_ldf.deflate_c(comp, p, n, z.data() + 18, 65536 - 26);
      if (c == 0) rc = Z_BUF_ERROR;        // did not fit: stored below
    } else {
      z_stream s{};
      deflateInit2(&s, level, Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY);
      s.next_in = (Bytef *)p;
      s.avail_in = (uInt)n;
      s.next_out = z.data() + 18;
      s.avail_out = (uInt)(z.size() - 26);
      rc = deflate(&s, Z_FINISH);
      c = z.size() - 26 - s.avail_out;
      deflateEnd(&s);
    }
    if (rc != Z_STREAM_END || c + 26 > 65536) {
      if (level) block(p, n, 0);   // incompressible: stored
      else ok = false;
      return;
    }
    const unsigned char h[18] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0,
                                 (unsigned char)((c + 25) & 255), (unsigned char)((c + 25) >> 8)};
    memcpy(z.data(), h, 18);
    const uint32_t crc = g_ldf.ok ? g_ldf.crc(0, p, n) : (uint32_t)crc32(0, (const Bytef *)p, (uInt)n);
    const uint32_t isz = (uint32_t)n;
    memcpy(z.data() + 18 + c, &crc, 4);
    memcpy(z.data() + 22 + c, &isz, 4);
    ok = ok && fwrite(z.data(), 1, c + 26, f) == c + 26;
  }
  void write(const char *p, size_t n) {
    while (n) {
      const size_t k = std::min(n, (size_t)65280 - blk.size());
      blk.insert(blk.end(), p, p + k);
      p += k;
      n -= k;
      if (blk.size() == 65280) {
        block(blk.data(), blk.size(), 1);
        blk.clear();
      }
    }
  }
  bool close() {
    if (!blk.empty()) block(blk.data(), blk.size(), 1);
    static const unsigned char eof[28] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43,
                                          2,    0,    0x1b, 0, 3, 0, 0, 0, 0, 0, 0,    0, 0, 0};
    ok = ok && fwrite(eof, 1, 28, f) == 28;
    return fclose(f) == 0 && ok;
  }
};

// The cohort's own BGZF encoder (the default for "bgzf"): a mosdepth line
// repeats the line before it up to the depth, but for the thousands digits of
// START and END -- so each line is compared with the one before, byte for
// byte: three copies around two literal digits, as a general compressor
// parses these lines, plus the depth's digits as literals, in ONE fixed
// dynamic-Huffman code written at the head of every block: about the size of
// libdeflate level 1's output at several times its rate.  Blocks hold 65280
// bytes of text each, lines cut where they cross, as htslib writes them.  GEN_COHORT_LIBDEFLATE=1: the general
// compressor above instead (the same text, other bytes).
struct FastCode {
  uint16_t lc[273], dc[16];               // bit-reversed codes
  uint8_t ll[273] = {0}, dl[16];
  uint32_t mbits[35];                     // match length 3..34: symbol code | extra << its length
  uint8_t mn[35];
  uint32_t dbits[257];                    // distance 1..256 likewise
  uint8_t dn[257];
  std::vector<std::pair<uint32_t, int>> head;   // the block header, LSB-first pieces
  static void canon(const uint8_t *len, int n, uint16_t *code) {
    int cnt[16] = {0}, next[16] = {0};
    for (int i = 0; i < n; i++) cnt[len[i]]++;
    cnt[0] = 0;
    for (int b = 1, c = 0; b < 16; b++) next[b] = c = (c + cnt[b - 1]) << 1;
    for (int i = 0; i < n; i++) {
      if (!len[i]) continue;
      const int v = next[len[i]]++;
      int r = 0;
      for (int b = 0; b < len[i]; b++) r |= ((v >> b) & 1) << (len[i] - 1 - b);
      code[i] = (uint16_t)r;
    }
  }
  FastCode() {
    // literal / length lengths: a complete code (Kraft sum 1)
    for (int c = '0'; c <= '9'; c++) ll[c] = 4;
    ll['.'] = 4;
    for (int c : {(int)'c', (int)'h', (int)'r', (int)'\t', (int)'\n', 256}) ll[c] = 7;
    for (int c = 257; c <= 268; c++) ll[c] = 6;
    ll[258] = ll[264] = ll[265] = 5;      // lengths 4, 10, 11-12: "000\t", "000\t123456", "\nchr1\t123456"
    for (int c = 269; c <= 272; c++) ll[c] = 7;
    // distance lengths, complete: one line back is 33-34 bytes (ten-digit positions), 25-32 before
    const uint8_t d[16] = {7, 7, 7, 7, 6, 6, 6, 4, 4, 2, 1, 6, 7, 7, 7, 7};
    memcpy(dl, d, 16);
    canon(ll, 273, lc);
    canon(dl, 16, dc);
    for (int n = 3; n <= 34; n++) {
      int sym, ex = 0, eb = 0;
      if (n <= 10) sym = 254 + n;
      else if (n <= 18) sym = 265 + (n - 11) / 2, ex = (n - 11) % 2, eb = 1;
      else sym = 269 + (n - 19) / 4, ex = (n - 19) % 4, eb = 2;
      mbits[n] = lc[sym] | (uint32_t)ex << ll[sym];
      mn[n] = (uint8_t)(ll[sym] + eb);
    }
    static const int base[16] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193};
    static const int ebits[16] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6};
    for (int v = 1; v <= 256; v++) {
      int c = 15;
      while (base[c] > v) c--;
      dbits[v] = dc[c] | (uint32_t)(v - base[c]) << dl[c];
      dn[v] = (uint8_t)(dl[c] + ebits[c]);
    }
    // BFINAL 1, BTYPE 10, HLIT 273, HDIST 16, HCLEN 19; the code-length code: 0..15 in 4 bits each
    head = {{1, 1}, {2, 2}, {273 - 257, 5}, {16 - 1, 5}, {19 - 4, 4}};
    static const int order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    uint8_t cl[19];
    uint16_t cc[19];
    for (int i = 0; i < 19; i++) cl[i] = i < 16 ? 4 : 0;
    canon(cl, 19, cc);
    for (int i = 0; i < 19; i++) head.push_back({cl[order[i]], 3});
    for (int i = 0; i < 273; i++) head.push_back({cc[ll[i]], 4});
    for (int i = 0; i < 16; i++) head.push_back({cc[dl[i]], 4});
  }
};
static const FastCode g_fc;

struct FastBgzf {
  FILE *f;
  unsigned char blk[65536 + 64];   // the block's text
  unsigned char z[65536 + 64];     // gzip member under construction (18-byte header first)
  int bl = 0;                      // text bytes in the block
  unsigned char *o = nullptr;
  uint64_t acc = 0;
  int nb = 0;
  int prev_s = -1;                 // the previous whole line's start in this block
  bool nl = false;                 // the last line's '\n' is in the text, not yet in the stream
  bool ok = true;
  explicit FastBgzf(FILE *ff) : f(ff) {}
  inline void put(uint64_t v, int b) {
    acc |= (uint64_t)v << nb;               // nb <= 7 here, b <= 56: no branch (its outcome has no pattern)
    nb += b;
    memcpy(o, &acc, 8);
    o += nb >> 3;
    acc >>= nb & ~7;
    nb &= 7;
  }
  inline void copy(int n, int dist) {          // 3 <= n <= 34, dist <= 256: at most 9 + 13 bits
    put(g_fc.mbits[n] | g_fc.dbits[dist] << g_fc.mn[n], g_fc.mn[n] + g_fc.dn[dist]);
  }
  // [p, end) of the block as copies of the text that starts at src (never if src < 0), else literals
  inline void seg(int p, int end, int src) {
    while (p < end) {
      int n = 0;
      if (src >= 0) {
        int mx = std::min(end - p, 34);
        while (n + 8 <= mx) {                 // eight bytes a step
          uint64_t x, y;
          memcpy(&x, blk + src + n, 8);
          memcpy(&y, blk + p + n, 8);
          if (x != y) { mx = n + (__builtin_ctzll(x ^ y) >> 3); break; }
          n += 8;
        }
        while (n < mx && blk[src + n] == blk[p + n]) n++;
      }
      if (n >= 3 && p - src <= 256) {
        copy(n, p - src);
      } else {
        n = 1;
        put(g_fc.lc[blk[p]], g_fc.ll[blk[p]]);
      }
      p += n;
      if (src >= 0) src += n;
    }
  }
  void flush() {
    if (!bl) return;
    if (nl) put(g_fc.lc['\n'], g_fc.ll['\n']);        // the last line's end
    nl = false;
    put(g_fc.lc[256], g_fc.ll[256]);
    if (nb > 0) *o++ = (unsigned char)acc;
    acc = 0;
    nb = 0;
    const size_t c = (size_t)(o - (z + 18));
    const unsigned char h[18] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0,
                                 (unsigned char)((c + 25) & 255), (unsigned char)((c + 25) >> 8)};
    memcpy(z, h, 18);
    const uint32_t crc = g_ldf.ok ? g_ldf.crc(0, blk, bl) : (uint32_t)crc32(0, (const Bytef *)blk, (uInt)bl);
    const uint32_t isz = (uint32_t)bl;
    memcpy(z + 18 + c, &crc, 4);
    memcpy(z + 22 + c, &isz, 4);
    ok = ok && c + 26 <= 65536 && fwrite(z, 1, c + 26, f) == c + 26;
    bl = 0;
    prev_s = -1;
  }
  void start() {
    o = z + 18;
    for (const auto &h : g_fc.head) put(h.first, h.second);
  }
  // one line (its '\n' last): START at ln + 5, ls digits; END after its tab, le digits; then tab, depth.
  // Blocks hold exactly 65280 bytes of text (as htslib cuts them): a line the block cannot take whole is cut.
  // plain: START and END differ from the line before's, and from each other, in the thousands digit only
  inline void line(const char *ln, int L, int ls, int le, bool plain) {
    const int fit = std::min(L, 65280 - bl);
    const int nd = L - 1 - (5 + ls + 1 + le + 1);         // the depth's characters
    if (plain && nl && prev_s > 0 && fit == L && L <= 48 && nd <= 7 && ls >= 4) {
      // the usual line, without the search: three copies one line back, the two stepped digits, the depth
      const int s = bl, dist = s - prev_s;
      memcpy(blk + s, ln, 48);
      bl += L;
      const FastCode &c = g_fc;
      const unsigned char *const u = (const unsigned char *)ln;
      uint64_t v = c.mbits[ls + 2];                        // "\nchr1\t" + START's head
      int n = c.mn[ls + 2];
      v |= (uint64_t)c.dbits[dist] << n, n += c.dn[dist];
      v |= (uint64_t)c.lc[u[5 + ls - 4]] << n, n += c.ll[u[5 + ls - 4]];
      put(v, n);
      v = c.mbits[le], n = c.mn[le];                       // "000\t" + END's head
      v |= (uint64_t)c.dbits[dist] << n, n += c.dn[dist];
      v |= (uint64_t)c.lc[u[5 + ls + 1 + le - 4]] << n, n += c.ll[u[5 + ls + 1 + le - 4]];
      put(v, n);
      v = c.mbits[4], n = c.mn[4];                         // "000\t"
      v |= (uint64_t)c.dbits[dist] << n, n += c.dn[dist];
      for (int k = L - 1 - nd; k < L - 1; k++) v |= (uint64_t)c.lc[u[k]] << n, n += c.ll[u[k]];
      put(v, n);                                           // <= 9 + 13 + 7 x 4 bits (digits and '.')
      prev_s = s;
      return;
    }
    if (fit > 0) {
      if (!bl) start();
      const int s = bl, lim = s + fit, e = std::min(s + L - 1, lim), d = std::min(s + 5 + ls + 1 + le + 1, lim);
      if (fit == L && L <= 48) memcpy(blk + s, ln, 48);     // (both buffers have the room)
      else memcpy(blk + s, ln, (size_t)fit);
      bl += fit;
      if (nl && prev_s > 0) {
        seg(s - 1, d, prev_s - 1);              // "\nchr1\t123456" | 7 | "000\t123456" | 8 | "000\t"
      } else {
        if (nl) put(g_fc.lc['\n'], g_fc.ll['\n']);
        seg(s, d, prev_s == 0 ? 0 : -1);        // (no '\n' before the block's first line)
      }
      seg(d, e, -1);                            // the depth
      nl = fit == L;                            // the line's own '\n' goes with the next line, or at the block's end
      prev_s = fit == L ? s : -1;
    }
    if (fit < L) {                              // the rest of the line opens the next block, as literals
      flush();
      start();
      bl = L - fit;
      memcpy(blk, ln + fit, (size_t)bl);
      seg(0, bl - 1, -1);
      nl = true;
    }
  }
  bool close() {
    flush();
    static const unsigned char eof[28] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43,
                                          2,    0,    0x1b, 0, 3, 0, 0, 0, 0, 0, 0,    0, 0, 0};
    ok = ok && fwrite(eof, 1, 28, f) == 28;
    return fclose(f) == 0 && ok;
  }
};

static inline char *put_u(char *o, uint64_t v) {
  char t[24];
  int k = 0;
  do { t[k++] = (char)('0' + v % 10); v /= 10; } while (v);
  while (k) *o++ = t[--k];
  return o;
}

int main(int argc, char **argv) {
  if (argc < 6) {
    fprintf(stderr, "usage: %s DIR N_SAMPLES N_BINS SEED THREADS [FIRST_SAMPLE]\n", argv[0]);
    return 2;
  }
  const std::string dir = argv[1];
  const int64_t n = atoll(argv[2]), m = atoll(argv[3]);
  const uint64_t seed = strtoull(argv[4], nullptr, 10);
  const int nt = atoi(argv[5]);
  const int64_t first = argc > 6 ? atoll(argv[6]) : 0;
  const bool bgzf = argc > 7 && !strcmp(argv[7], "bgzf");
  const int ncl = 26;
  // per-bin parts, shared by every sample (the cluster offsets cluster by cluster)
  std::vector<float> base(m), off((size_t)m * ncl);
  {
    std::vector<std::thread> th;
    for (int t = 0; t < nt; t++)
      th.emplace_back([&, t]() {
        for (int64_t b = t; b < m; b += nt) {
          base[b] = 25.0f + 30.0f * unif(mix(seed ^ ((uint64_t)b * 0x9E37ull) ^ 0x1234ull));
          for (int c = 0; c < ncl; c++)
            off[(size_t)c * m + b] = 0.16f * (unif(mix(seed ^ ((uint64_t)b << 8) ^ (uint64_t)c ^ 0x77ull)) - 0.5f);
        }
      });
    for (auto &t : th) t.join();
  }
  const bool dry = getenv("GEN_COHORT_DRY") != nullptr;   // timing: text only, nothing compressed or written
  const bool fast = bgzf && !dry && getenv("GEN_COHORT_LIBDEFLATE") == nullptr;
  std::atomic<int64_t> next{0}, failed{0}, done{0};
  auto work = [&]() {
    std::vector<char> buf(1 << 20);
    for (;;) {
      const int64_t i = first + next++;
      if (i >= first + n) break;
      const uint64_t hs = mix(seed ^ (0xA5A5ull << 48) ^ (uint64_t)i);
      const int c = (int)(mix(hs) % (uint64_t)ncl);
      const float scale = 0.6f + 0.8f * unif(hs);
      char path[4096];
      snprintf(path, sizeof path, "%s/S%05lld.regions.bed.gz", dir.c_str(), (long long)i);
      gzFile f = nullptr;
      Bgzf *bw = nullptr;
      FastBgzf *fw = nullptr;
      if (fast) {
        FILE *ff = fopen(path, "wb");
        if (!ff) { failed++; continue; }
        setvbuf(ff, nullptr, _IOFBF, 1 << 20);
        fw = new FastBgzf(ff);
      } else if (bgzf) {
        FILE *ff = fopen(path, "wb");
        if (!ff) { failed++; continue; }
        bw = new Bgzf(ff);
      } else {
        f = gzopen(path, "wb1");
        if (!f) { failed++; continue; }
        gzbuffer(f, 1 << 20);
      }
      auto emit = [&](const char *p, size_t k) {
        if (dry) return;
        if (bw) bw->write(p, k);
        else gzwrite(f, p, (unsigned)k);
      };
      size_t pos = 0;
      const float *const offc = off.data() + (size_t)c * m;      // this sample's cluster, bin by bin
      char sd[24], ed[24];                     // START and END as digits, END stepped by 1000 per line
      int ls = 0, le = (int)(put_u(ed, 0) - ed);
      bool stepped = false;                    // the line before: END = START but for the thousands digit
      for (int64_t b = 0; b < m; b++) {
        const uint64_t h = mix(seed ^ ((uint64_t)i << 40) ^ (uint64_t)b);
        const float u1 = unif(h), u2 = (float)((h >> 16) & 0xFFFFFFull) * (1.0f / 16777216.0f);
        const uint32_t lo = (uint32_t)(h & 0xFFFFull);
        const float u3 = (float)lo * (1.0f / 65536.0f);
        float cnv = 1.0f;
        if (u3 < 0.02f) cnv = (u3 < 0.01f) ? 0.5f : 1.5f;
        const float spike = (lo == 0x2A2Au) ? 40.0f : 1.0f;
        const float noise = 1.0f + 0.2f * (u1 + u2 - 1.0f);
        const float d = base[b] * (1.0f + offc[b]) * scale * cnv * noise * spike;
        const int32_t q = (int32_t)rintf(d * 100.0f);
        if (pos + 64 > buf.size()) { emit(buf.data(), pos); pos = 0; }
        char *o = buf.data() + pos;
        char *const l0 = o;
        memcpy(o, "chr1\t", 5);
        o += 5;
        memcpy(sd, ed, 16);                    // (<= 10 digits; fixed sizes copy inline)
        ls = le;
        int k = le - 4;                        // the thousands digit
        if (k < 0) {
          k = -2;
          le = (int)(put_u(ed, (uint64_t)(b * 1000 + 1000)) - ed);
        } else {
          while (k >= 0 && ed[k] == '9') ed[k--] = '0';
          if (k >= 0) ed[k]++;
          else { memmove(ed + 1, ed, (size_t)le); ed[0] = '1'; le++; }
        }
        memcpy(o, sd, 16);
        o += ls;
        *o++ = '\t';
        memcpy(o, ed, 16);
        o += le;
        *o++ = '\t';
        o = put_u(o, (uint64_t)(q / 100));
        *o++ = '.';
        *o++ = (char)('0' + (q % 100) / 10);
        *o++ = (char)('0' + q % 10);
        *o++ = '\n';
        if (fw) {
          const bool step = k == le - 4 && ls == le;       // END = START but for the thousands digit
          fw->line(l0, (int)(o - l0), ls, le, step && stepped);
          stepped = step;
        }
        else pos = (size_t)(o - buf.data());
      }
      if (pos) emit(buf.data(), pos);
      if (fw) {
        if (!fw->close()) failed++;
        delete fw;
      } else if (bw) {
        if (!bw->close()) failed++;
        delete bw;
      } else if (gzclose(f) != Z_OK) {
        failed++;
      }
      const int64_t d = ++done;
      if (d % 200 == 0 || d == n) {          // progress for a caller's watchdog
        fprintf(stderr, "[gen_cohort] %lld of %lld files\n", (long long)d, (long long)n);
        fflush(stderr);
      }
    }
  };
  std::vector<std::thread> th;
  for (int t = 0; t < nt; t++) th.emplace_back(work);
  for (auto &t : th) t.join();
  if (failed) {
    fprintf(stderr, "%lld files failed\n", (long long)failed.load());
    return 1;
  }
  return 0;
}
