// What the lanes of flac_kernel (csrc/ptts_flac.hip) do with ptts_flac.h, as a plain program on heap buffers of exactly the
// size each step may touch, for a sanitizer build: the cut of a block from the previous and the current line, the per-lane
// sums, the choice, the lanes' consecutive residual ranges, the exclusive scan of their code lengths, the ORs into the bit
// buffer (sized to the frame's last word: a mask that falls behind it is an error), the per-lane CRCs and their combination.
//
// usage: flac_sweep CASES.bin > FRAMES.bin
//   CASES.bin   int32 count, then per case int32 {n, preroll, first_block, rate, lines} and lines * n int16 samples
//   FRAMES.bin  per case and line: uint32 nbytes (0 while the row leads), then the frame's bytes
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "ptts_flac.h"

static const int T = PTTS_FL_LANES;

static void put(uint32_t *buf, size_t words, uint32_t p, uint32_t v, int L) {
  uint32_t w, m0, m1;
  fl_split(p, v, L, &w, &m0, &m1);
  (void)words;
  if (m0) buf[w] |= m0;  // out of bounds here is the sanitizer's to report
  if (m1) buf[w + 1] |= m1;
}

static std::vector<uint8_t> encode_block(const int16_t *prev, const int16_t *cur, int n, int off, uint32_t number, int rate,
                                         const uint8_t *t8, const uint16_t *t16) {
  std::unique_ptr<int32_t[]> x(new int32_t[n]);
  for (int i = 0; i < n; ++i) x[i] = fl_cut(prev, cur, n, off, i);
  bool constant = true;
  for (int i = 0; i < n; ++i) constant &= x[i] == x[0];
  int type = PTTS_FL_CONSTANT, o = 0, k = 0;
  if (!constant) {
    std::unique_ptr<uint64_t[]> sums(new uint64_t[PTTS_FL_SUMS]());
    for (int t = 0; t < T; ++t) {  // lane t: samples t, t + T, ..; its partial sums stay below 2^32
      uint32_t acc[PTTS_FL_ORDERS][PTTS_FL_KS] = {};
      for (int i = t; i < n; i += T)
        for (int oo = 0; oo < PTTS_FL_ORDERS; ++oo) {
          if (i < oo) continue;
          const uint32_t u = fl_fold(fl_resid(x.get(), i, oo));
          for (int kk = 0; kk < PTTS_FL_KS; ++kk) {
            if (acc[oo][kk] > 0xFFFFFFFFu - (u >> kk)) { fprintf(stderr, "a lane's partial sum overflows\n"); exit(2); }
            acc[oo][kk] += u >> kk;
          }
        }
      for (int s = 0; s < PTTS_FL_SUMS; ++s) sums[s] += acc[s / PTTS_FL_KS][s % PTTS_FL_KS];
    }
    type = fl_choose(sums.get(), n, &o, &k);
  }
  uint8_t h[PTTS_FL_HEADER_MAX];
  const int hlen = fl_header(h, number, n, rate, t8);
  const uint32_t sub = 8u * (uint32_t)hlen;
  // the lanes' lengths and their exclusive scan
  std::vector<uint32_t> start(T, 0);
  uint32_t total_bits;
  if (type == PTTS_FL_CONSTANT) total_bits = sub + 24u;
  else if (type == PTTS_FL_VERBATIM) total_bits = sub + 8u + 16u * (uint32_t)n;
  else {
    uint32_t run = 0;
    for (int t = 0; t < T; ++t) {
      int lo, hi;
      fl_range(t, n - o, &lo, &hi);
      start[t] = run;
      for (int r = lo; r < hi; ++r) run += (fl_fold(fl_resid(x.get(), o + r, o)) >> k) + 1u + (uint32_t)k;
    }
    total_bits = fl_codes_at(hlen, o) + run;
  }
  const uint32_t body = (total_bits + 7u) / 8u, nbytes = body + 2u;
  if ((int)nbytes > fl_frame_max(n)) { fprintf(stderr, "frame of %u bytes for n = %d\n", nbytes, n); exit(2); }
  const size_t words = (nbytes + 3u) / 4u;
  std::unique_ptr<uint32_t[]> buf(new uint32_t[words]());
  for (int i = 0; i < hlen; ++i) put(buf.get(), words, 8u * i, h[i], 8);
  if (type == PTTS_FL_CONSTANT) {
    put(buf.get(), words, sub + 8u, (uint32_t)x[0] & 0xFFFFu, 16);
  } else if (type == PTTS_FL_VERBATIM) {
    put(buf.get(), words, sub, 0x02u, 8);
    for (int i = 0; i < n; ++i) put(buf.get(), words, sub + 8u + 16u * (uint32_t)i, (uint32_t)x[i] & 0xFFFFu, 16);
  } else {
    put(buf.get(), words, sub, 0x10u | ((uint32_t)o << 1), 8);
    put(buf.get(), words, sub + 8u + 16u * (uint32_t)o, (uint32_t)k, 10);
    for (int t = 0; t < o; ++t) put(buf.get(), words, sub + 8u + 16u * (uint32_t)t, (uint32_t)x[t] & 0xFFFFu, 16);
    for (int t = T - 1; t >= 0; --t) {  // any order of the lanes gives the same words
      int lo, hi;
      fl_range(t, n - o, &lo, &hi);
      uint32_t p = fl_codes_at(hlen, o) + start[t];
      for (int r = lo; r < hi; ++r) {
        uint32_t zeros, v;
        int L;
        fl_code(fl_fold(fl_resid(x.get(), o + r, o)), k, &zeros, &v, &L);
        put(buf.get(), words, p + zeros, v, L);
        p += zeros + (uint32_t)L;
      }
    }
  }
  uint32_t crc = 0;
  for (int t = 0; t < T; ++t) {
    int lo, hi;
    fl_range(t, (int)body, &lo, &hi);
    uint16_t c = 0;
    for (int j = lo; j < hi; ++j) c = fl_crc16(t16, c, fl_byte(buf.get(), (uint32_t)j));
    if (hi > lo) crc ^= fl_gfmul16(c, fl_xpow8(body - (uint32_t)hi));
  }
  put(buf.get(), words, 8u * body, crc & 0xFFFFu, 16);
  std::vector<uint8_t> out(nbytes);
  for (uint32_t j = 0; j < nbytes; ++j) out[j] = fl_byte(buf.get(), j);
  return out;
}

int main(int argc, char **argv) {
  if (argc != 2) { fprintf(stderr, "usage: flac_sweep CASES.bin\n"); return 2; }
  FILE *f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  std::unique_ptr<uint8_t[]> t8(new uint8_t[256]);
  std::unique_ptr<uint16_t[]> t16(new uint16_t[256]);
  for (int b = 0; b < 256; ++b) { t8[b] = fl_crc8_entry(b); t16[b] = fl_crc16_entry(b); }
  int32_t count = 0;
  if (fread(&count, 4, 1, f) != 1) return 2;
  for (int c = 0; c < count; ++c) {
    int32_t hd[5];
    if (fread(hd, 4, 5, f) != 5) return 2;
    const int n = hd[0], preroll = hd[1], first = hd[2], rate = hd[3], lines = hd[4];
    if (n < PTTS_FL_MIN_N || n > PTTS_FL_MAX_N || preroll < 0 || lines < 0) return 2;
    const int off = preroll % n, lead = (preroll + n - 1) / n;
    std::unique_ptr<int16_t[]> prev(new int16_t[n]()), cur(new int16_t[n]);
    for (int line = 0; line < lines; ++line) {
      if (fread(cur.get(), 2, n, f) != (size_t)n) return 2;
      uint32_t nbytes = 0;
      std::vector<uint8_t> frame;
      if (line >= lead) {
        frame = encode_block(prev.get(), cur.get(), n, off, (uint32_t)first + (uint32_t)(line - lead), rate, t8.get(), t16.get());
        nbytes = (uint32_t)frame.size();
      }
      fwrite(&nbytes, 4, 1, stdout);
      if (nbytes) fwrite(frame.data(), 1, nbytes, stdout);
      memcpy(prev.get(), cur.get(), 2 * (size_t)n);
    }
  }
  fclose(f);
  return 0;
}
