// Host sweep of csrc/ptts_encode.h (tests/test_encoding_cpu.py compiles it with AddressSanitizer and UBSan).
//   stdout: en_mulaw(s) for s = -32768 .. 32767, en_alaw(s) likewise, then en_s16(x) of the ramp x = (s +- 0.5) / 32767,
//           s = -32767 .. 32767, as little-endian int16
//   stderr: "ok" after the index sweep: for widths and n that cover every branch (n = 1, n = width, widths that are no
//           multiple of 4 or 16), every run of every row does on exact-size heap buffers what the kernel's lanes do - full
//           runs as whole 16-byte blocks, the run with the row's end sample by sample, runs past it nothing - and each row holds
//           exactly n * bytes_per_sample converted bytes followed by untouched ones.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ptts_encode.h"

static void put(uint8_t *o, int code, int i, float x) {
  const int s = en_s16(x);
  if (code == 1) memcpy(o + 4 * i, &x, 4);
  else if (code == 0) { o[2 * i] = (uint8_t)(s & 0xFF); o[2 * i + 1] = (uint8_t)((s >> 8) & 0xFF); }
  else o[i] = code == 2 ? en_mulaw(s) : en_alaw(s);
}

static int sweep(int B, int width) {
  const int64_t pitch = en_pitch(width);
  if (pitch % 16 || pitch < 4 * (int64_t)width) return 1;
  float *in = (float *)malloc(sizeof(float) * B * width);
  uint8_t *out = (uint8_t *)malloc((size_t)(B * pitch));
  for (int i = 0; i < B * width; ++i) in[i] = (float)((i * 37) % 2001 - 1000) / 900.0f;
  const int ns[] = {1, 2, 3, 5, 15, 16, 17, width - 1, width};
  int bad = 0;
  for (int n : ns) {
    if (n < 1 || n > width) continue;
    for (int code = 0; code < PTTS_EN_CODES; ++code) {
      memset(out, 0xA5, (size_t)(B * pitch));
      const int bps = en_bps(code);
      for (int row = 0; row < B; ++row)
        for (int r = 0; r < en_runs(width) + 3; ++r) {  // the grid is rounded up to whole blocks: lanes past the last run
          const int tail = en_tail(r, n);
          if (tail <= 0) continue;
          const float *x = in + (size_t)row * width + (size_t)PTTS_EN_RUN * r;
          uint8_t *o = out + (size_t)row * pitch + (size_t)PTTS_EN_RUN * r * bps;
          if (!en_full(r, n)) {
            for (int i = 0; i < tail; ++i) put(o, code, i, x[i]);
            continue;
          }
          uint8_t block[PTTS_EN_RUN * 4];
          for (int i = 0; i < PTTS_EN_RUN; ++i) put(block, code, i, x[i]);
          if ((o - out) % 16) ++bad;                        // every whole store is aligned
          for (int q = 0; q < bps; ++q) memcpy(o + 16 * q, block + 16 * q, 16);  // bps stores of 16 bytes
        }
      for (int row = 0; row < B; ++row) {
        std::vector<uint8_t> want((size_t)pitch, 0xA5);
        for (int i = 0; i < n; ++i) put(want.data(), code, i, in[(size_t)row * width + i]);
        if (memcmp(want.data(), out + (size_t)row * pitch, (size_t)pitch)) ++bad;
      }
    }
  }
  free(in);
  free(out);
  return bad;
}

int main() {
  for (int s = -32768; s <= 32767; ++s) putchar(en_mulaw(s));
  for (int s = -32768; s <= 32767; ++s) putchar(en_alaw(s));
  for (int s = -32767; s <= 32767; ++s) {
    const float x = (float)((s >= 0 ? s + 0.5 : s - 0.5) / 32767.0);
    const int16_t v = (int16_t)en_s16(x);
    putchar(v & 0xFF);
    putchar((v >> 8) & 0xFF);
  }
  int bad = 0;
  const int widths[] = {1, 3, 16, 17, 882, 1920, 1921};
  for (int w : widths) bad += sweep(3, w);
  fprintf(stderr, bad ? "bad %d\n" : "ok\n", bad);
  return bad != 0;
}
