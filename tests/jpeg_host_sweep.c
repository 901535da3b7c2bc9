/* Stand-alone sanitizer sweep of the host JPEG parser (csrc/jpeg_host.c): built by tests/test_jpeg_craft.py together
 * with the parser under -fsanitize=address,undefined and run as a child process - never loaded into an interpreter.
 *
 * For every file named on the command line: vis_jpeg_probe, and on success vis_jpeg_decode_coeffs into a heap buffer of
 * EXACTLY total_blocks * 64 int16 (one write past it is a sanitizer report), over
 *   every prefix of the file;
 *   every single-byte substitution with 0x00, 0xFF, one flipped bit and one pseudo-random byte;
 *   every single-byte deletion;
 *   N pseudo-random multi-byte mutations per file (--random N, default 20000).
 * Each input is a fresh heap copy of exactly its length, so a read past the end is a report too.  The info struct is
 * pre-filled with 0xA5 before every probe.  Prints the counts; exit status 0 unless a sanitizer stops the program. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "vis_jpeg_host.h"

static unsigned long long n_ok, n_unsupported, n_corrupt, n_decoded, n_range, n_decode_corrupt;
static uint32_t lcg_state = 12345u;

static uint32_t lcg(void) {
  lcg_state = lcg_state * 1664525u + 1013904223u;
  return lcg_state >> 8;
}

static void run_one(const uint8_t* src, size_t n) {
  uint8_t* d = (uint8_t*)malloc(n ? n : 1);  /* exact size: the redzone starts at d + n */
  if (!d) exit(2);
  memcpy(d, src, n);
  VisJpegInfo info;
  memset(&info, 0xA5, sizeof(info));
  const int rc = vis_jpeg_probe(d, n, &info);
  if (rc == 0) {
    ++n_ok;
    if (info.total_blocks <= 0 || info.total_blocks > (1 << 21)) {
      fprintf(stderr, "probe accepted total_blocks = %d\n", info.total_blocks);
      exit(3);
    }
    int16_t* coeffs = (int16_t*)malloc((size_t)info.total_blocks * 64 * sizeof(int16_t));
    if (!coeffs) exit(2);
    const int rd = vis_jpeg_decode_coeffs(d, n, &info, coeffs);
    if (rd == 0) ++n_decoded;
    else if (rd == -3) ++n_range;
    else ++n_decode_corrupt;
    free(coeffs);
  } else if (rc == -1) {
    ++n_unsupported;
  } else {
    ++n_corrupt;
  }
  free(d);
}

static void sweep(const uint8_t* f, size_t n, long random_count) {
  uint8_t* m = (uint8_t*)malloc(n + 1);
  if (!m) exit(2);
  for (size_t k = 0; k <= n; ++k) run_one(f, k);                 /* every prefix, the whole file last */
  for (size_t i = 0; i < n; ++i) {                               /* substitutions */
    const uint8_t subs[4] = {0x00, 0xFF, (uint8_t)(f[i] ^ (1u << (lcg() & 7))), (uint8_t)lcg()};
    for (int s = 0; s < 4; ++s) {
      memcpy(m, f, n);
      m[i] = subs[s];
      run_one(m, n);
    }
  }
  for (size_t i = 0; i < n; ++i) {                               /* deletions */
    memcpy(m, f, i);
    memcpy(m + i, f + i + 1, n - i - 1);
    run_one(m, n - 1);
  }
  for (long r = 0; r < random_count; ++r) {                      /* 1..8 bytes changed anywhere */
    memcpy(m, f, n);
    const int cnt = 1 + (int)(lcg() & 7);
    for (int c = 0; c < cnt; ++c) m[lcg() % n] = (uint8_t)lcg();
    run_one(m, n);
  }
  free(m);
}

int main(int argc, char** argv) {
  long random_count = 20000;
  int files = 0;
  for (int a = 1; a < argc; ++a) {
    if (!strcmp(argv[a], "--random") && a + 1 < argc) {
      random_count = atol(argv[++a]);
      continue;
    }
    FILE* fp = fopen(argv[a], "rb");
    if (!fp) {
      fprintf(stderr, "cannot open %s\n", argv[a]);
      return 2;
    }
    fseek(fp, 0, SEEK_END);
    const long sz = ftell(fp);
    fseek(fp, 0, SEEK_SET);
    if (sz <= 0) return 2;
    uint8_t* f = (uint8_t*)malloc((size_t)sz);
    if (!f || fread(f, 1, (size_t)sz, fp) != (size_t)sz) return 2;
    fclose(fp);
    sweep(f, (size_t)sz, random_count);
    free(f);
    ++files;
  }
  printf("files=%d ok=%llu unsupported=%llu corrupt=%llu decoded=%llu range=%llu decode_corrupt=%llu\n", files, n_ok,
         n_unsupported, n_corrupt, n_decoded, n_range, n_decode_corrupt);
  return files ? 0 : 2;
}
