/*
 * host_reader_formats.c -- rdsp_iq_reader_t on recordings in the engine's source formats (csrc/rdsp_io.c), as a program of its
 * own for a build with -fsanitize=address,undefined: it writes RAW .cu8 / .cs8 / .cf32 and WAV 8-bit / float32 (plain and
 * through the extensible header) files into the directory it is given, reads them back through rdsp_iq_reader_open_samples /
 * _read_samples with exactly sized buffers, and walks the refusals (WAV 24-bit, mono, a sample format that contradicts the
 * header, rdsp_iq_reader_read on a reader that is not int16).  Prints "host_reader_formats OK".
 */
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "rdsp.h"

static char g_err[512];
void rdsp_set_error(const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof g_err, fmt, ap);
  va_end(ap);
}
const char *rdsp_last_error(void) { return g_err; }

static int fails = 0;
#define CHECK(c) do { if (!(c)) { printf("FAIL line %d: %s (%s)\n", __LINE__, #c, g_err); fails++; } } while (0)

#define N_PAIRS 301 /* odd, and no multiple of the read size below */

static size_t pair_bytes(int fmt) { return fmt == RDSP_SRC_F32 ? 8u : fmt == RDSP_SRC_S16 ? 4u : 2u; }

/* element k (I and Q interleaved) of the test recording in format fmt, written into p */
static void element(int fmt, size_t k, unsigned char *p) {
  if (fmt == RDSP_SRC_U8) p[0] = (unsigned char)(k * 7u + 3u);
  else if (fmt == RDSP_SRC_S8) p[0] = (unsigned char)(int8_t)((int)(k * 5u % 256u) - 128);
  else if (fmt == RDSP_SRC_S16) { const int16_t v = (int16_t)((int)(k * 211u % 65536u) - 32768); memcpy(p, &v, 2); }
  else { const float v = ((float)(k % 97u) - 48.0f) / 64.0f; memcpy(p, &v, 4); }
}
static unsigned char *recording(int fmt, size_t *bytes) {
  const size_t eb = pair_bytes(fmt) / 2;
  *bytes = N_PAIRS * 2 * eb;
  unsigned char *b = (unsigned char *)malloc(*bytes);
  for (size_t k = 0; b && k < 2 * (size_t)N_PAIRS; k++) element(fmt, k, b + k * eb);
  return b;
}
static void put16(unsigned char *p, unsigned v) { p[0] = (unsigned char)v; p[1] = (unsigned char)(v >> 8); }
static void put32(unsigned char *p, uint32_t v) { put16(p, v & 0xffffu); put16(p + 2, v >> 16); }

/* RIFF/WAVE with a 16-byte fmt chunk, or the 40-byte extensible one whose sub-format starts with the tag */
static int write_wav(const char *path, unsigned tag, unsigned nch, unsigned bits, uint32_t rate, int extensible, const unsigned char *data, size_t bytes) {
  unsigned char h[68];
  const uint32_t fmt_size = extensible ? 40u : 16u;
  memset(h, 0, sizeof h);
  memcpy(h, "RIFF", 4); put32(h + 4, 4u + 8u + fmt_size + 8u + (uint32_t)bytes); memcpy(h + 8, "WAVEfmt ", 8); put32(h + 16, fmt_size);
  put16(h + 20, extensible ? 0xFFFEu : tag); put16(h + 22, nch); put32(h + 24, rate); put32(h + 28, rate * nch * bits / 8u);
  put16(h + 32, nch * bits / 8u); put16(h + 34, bits);
  if (extensible) { put16(h + 36, 22); put16(h + 38, bits); put32(h + 40, 3); put16(h + 44, tag); }
  unsigned char *d = h + 20 + fmt_size;
  memcpy(d, "data", 4); put32(d + 4, (uint32_t)bytes);
  FILE *f = fopen(path, "wb");
  if (!f) return -1;
  const size_t hn = 20 + fmt_size + 8;
  const int ok = fwrite(h, 1, hn, f) == hn && fwrite(data, 1, bytes, f) == bytes;
  return fclose(f) == 0 && ok ? 0 : -1;
}
static int write_raw(const char *path, const unsigned char *data, size_t bytes) {
  FILE *f = fopen(path, "wb");
  if (!f) return -1;
  const int ok = fwrite(data, 1, bytes, f) == bytes;
  return fclose(f) == 0 && ok ? 0 : -1;
}

/* open, compare format / rate / frames, read it back in pieces of 64 pairs into exactly sized buffers */
static void read_back(const char *path, int container, int ask, int fmt, double rate, const unsigned char *want) {
  rdsp_iq_reader_t *r = NULL;
  CHECK(rdsp_iq_reader_open_samples(path, container, ask, &r) == RDSP_OK && r);
  if (!r) return;
  CHECK(rdsp_iq_reader_sample_format(r) == fmt);
  CHECK(rdsp_iq_reader_sample_rate(r) == rate);
  CHECK(rdsp_iq_reader_frames(r) == N_PAIRS);
  const size_t pb = pair_bytes(fmt);
  size_t at = 0;
  for (;;) {
    unsigned char *buf = (unsigned char *)malloc(64 * pb);
    const size_t got = rdsp_iq_reader_read_samples(r, buf, 64);
    CHECK(got <= 64 && at + got <= N_PAIRS && memcmp(buf, want + at * pb, got * pb) == 0);
    free(buf);
    at += got;
    if (got < 64) break;
  }
  CHECK(at == N_PAIRS);
  if (fmt != RDSP_SRC_S16) {
    int16_t one[2] = {7, 7};
    g_err[0] = 0;
    CHECK(rdsp_iq_reader_read(r, one, 1) == 0 && strstr(g_err, "not int16") && one[0] == 7);
  }
  rdsp_iq_reader_close(r);
}

int main(int argc, char **argv) {
  if (argc != 2) { fprintf(stderr, "usage: host_reader_formats DIR\n"); return 2; }
  char path[1024];
  static const char *const ext[4] = {"cs16", "cu8", "cs8", "cf32"};
  for (int fmt = RDSP_SRC_S16; fmt <= RDSP_SRC_F32; fmt++) {
    size_t bytes;
    unsigned char *data = recording(fmt, &bytes);
    if (!data) return 2;
    snprintf(path, sizeof path, "%s/c_rec.%s", argv[1], ext[fmt]);
    CHECK(write_raw(path, data, bytes) == 0);
    read_back(path, RDSP_IO_RAW, fmt, fmt, 0.0, data);
    read_back(path, RDSP_IO_AUTO, fmt, fmt, 0.0, data);
    if (fmt != RDSP_SRC_S8) { /* WAV has no signed 8-bit */
      const unsigned tag = fmt == RDSP_SRC_F32 ? 3u : 1u, bits = (unsigned)pair_bytes(fmt) * 4u;
      for (int x = 0; x < 2; x++) {
        snprintf(path, sizeof path, "%s/c_rec_%s_%d.wav", argv[1], ext[fmt], x);
        CHECK(write_wav(path, tag, 2, bits, 2400000u, x, data, bytes) == 0);
        read_back(path, RDSP_IO_WAV, -1, fmt, 2400000.0, data);
        read_back(path, RDSP_IO_AUTO, fmt, fmt, 2400000.0, data);
        for (int other = RDSP_SRC_S16; other <= RDSP_SRC_F32; other++) { /* a sample format that contradicts the header */
          rdsp_iq_reader_t *r = NULL;
          if (other != fmt) CHECK(rdsp_iq_reader_open_samples(path, RDSP_IO_WAV, other, &r) == RDSP_ERR_UNSUPPORTED && !r);
        }
        rdsp_iq_reader_t *r = NULL; /* the int16 entry point keeps its behaviour */
        const int rc = rdsp_iq_reader_open(path, RDSP_IO_AUTO, &r);
        CHECK(fmt == RDSP_SRC_S16 ? rc == RDSP_OK && r : rc == RDSP_ERR_UNSUPPORTED && !r && strstr(g_err, "need PCM 16-bit stereo"));
        rdsp_iq_reader_close(r);
      }
    }
    free(data);
  }
  { /* refused: 24-bit PCM, mono 8-bit, float64, an unknown sample format */
    unsigned char z[48] = {0};
    rdsp_iq_reader_t *r = NULL;
    snprintf(path, sizeof path, "%s/c_bad.wav", argv[1]);
    CHECK(write_wav(path, 1, 2, 24, 48000u, 0, z, 48) == 0);
    CHECK(rdsp_iq_reader_open_samples(path, RDSP_IO_WAV, -1, &r) == RDSP_ERR_UNSUPPORTED && !r && strstr(g_err, "24 bits"));
    CHECK(write_wav(path, 1, 1, 8, 48000u, 0, z, 48) == 0);
    CHECK(rdsp_iq_reader_open_samples(path, RDSP_IO_WAV, -1, &r) == RDSP_ERR_UNSUPPORTED && !r && strstr(g_err, "1 channels"));
    CHECK(rdsp_iq_reader_open_samples(path, RDSP_IO_WAV, RDSP_SRC_U8, &r) == RDSP_ERR_UNSUPPORTED && !r);
    CHECK(write_wav(path, 3, 2, 64, 48000u, 1, z, 48) == 0);
    CHECK(rdsp_iq_reader_open_samples(path, RDSP_IO_WAV, -1, &r) == RDSP_ERR_UNSUPPORTED && !r);
    CHECK(rdsp_iq_reader_open_samples(path, RDSP_IO_RAW, 4, &r) == RDSP_ERR_INVALID && !r);
    CHECK(rdsp_iq_reader_open_samples(path, RDSP_IO_RAW, -2, &r) == RDSP_ERR_INVALID && !r);
    CHECK(rdsp_iq_reader_sample_format(NULL) == RDSP_ERR_INVALID && rdsp_iq_reader_read_samples(NULL, z, 1) == 0);
  }
  if (fails) return 1;
  printf("host_reader_formats OK\n");
  return 0;
}
