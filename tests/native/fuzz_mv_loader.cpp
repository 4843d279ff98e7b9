// Host-side robustness driver for the multi-vector index's snapshot loader and the argument checks
// of sr_mv_save / sr_mv_load / sr_mv_compact, built by `make -C super-rag_amd asan_mv` with
// AddressSanitizer + UndefinedBehaviorSanitizer on the HOST code only (the objects of the `asan`
// target; no GPU needed) and run by tests/test_native_asan_mv.py:
//   * sr_mv_load on every truncation of a valid fp16 and a valid fp8 snapshot (3 rows, one without
//     tokens, one dead), on a trailing byte, a missing and an empty file, a bad magic, every header
//     rule (values near 2^31, 2^40, 2^62 and negatives), broken offsets, live bytes and fp8 NaN
//     codes, and on 400 seeded random bit flips of the 32 header bytes: each must return SR_ERR_IO
//     before anything is allocated (the flips: anything but SR_OK without a device); a valid
//     snapshot gets past the parser and fails only at the missing device;
//   * null and invalid arguments: each must return an SR_ERR_* code.
// Any out-of-bounds access, overflow or misaligned load aborts the run with a sanitizer report.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "super_rag_mi355x.h"

static int g_cases = 0, g_fail = 0;

static void expect(bool ok, const std::string& what, int rc) {
  ++g_cases;
  if (!ok) {
    ++g_fail;
    std::fprintf(stderr, "FAIL: %s (rc %d, last error: %s)\n", what.c_str(), rc, sr_last_error());
  }
}

template <class T>
static void put(std::vector<uint8_t>& b, T v) {
  const uint8_t* p = reinterpret_cast<const uint8_t*>(&v);
  b.insert(b.end(), p, p + sizeof(T));
}

template <class T>
static std::vector<uint8_t> patched(std::vector<uint8_t> b, size_t at, T v) {
  std::memcpy(b.data() + at, &v, sizeof(T));
  return b;
}

static void write_file(const std::string& path, const std::vector<uint8_t>& bytes) {
  FILE* f = std::fopen(path.c_str(), "wb");
  if (!f) {
    std::perror(path.c_str());
    std::exit(2);
  }
  if (!bytes.empty()) std::fwrite(bytes.data(), 1, bytes.size(), f);
  std::fclose(f);
}

// "SRMIMVX1", int32 dim, int32 dtype, int64 n_rows, int64 n_tokens, n_rows + 1 offsets, n_rows live
// bytes, the pool (multivec.hip MultiVecIndex::save): rows of 2 / 0 / 1 tokens, the last one dead
static const int kDim = 64;
static const int64_t kRows = 3, kTokens = 3;
static const size_t kOffAt = 32, kLiveAt = kOffAt + 8 * (kRows + 1), kPoolAt = kLiveAt + kRows;

static std::vector<uint8_t> snapshot(int32_t dtype) {
  std::vector<uint8_t> b;
  const char* m = "SRMIMVX1";
  b.insert(b.end(), m, m + 8);
  put<int32_t>(b, kDim);
  put<int32_t>(b, dtype);
  put<int64_t>(b, kRows);
  put<int64_t>(b, kTokens);
  for (int64_t o : {0, 2, 2, 3}) put<int64_t>(b, o);
  for (uint8_t l : {1, 1, 0}) b.push_back(l);
  const size_t n = (size_t)kTokens * kDim;
  if (dtype == SR_DTYPE_FP8_E4M3)
    for (size_t i = 0; i < n; ++i) b.push_back((uint8_t)((i * 37) % 0x7f | (i % 3 == 0 ? 0x80 : 0)));  // no NaN code
  else
    for (size_t i = 0; i < n; ++i) put<uint16_t>(b, (uint16_t)(0x2c00 + (i % 11)));  // ~1/16
  return b;
}

static int load(const std::string& p) {
  sr_mv* x = nullptr;
  const int rc = sr_mv_load(p.c_str(), 0, &x);
  if (x) sr_mv_destroy(x);
  return rc;
}

int main(int argc, char** argv) {
  const std::string dir = argc > 1 ? argv[1] : ".";
  const std::string path = dir + "/fuzz.srmv";
  int ndev = -1;
  expect(sr_device_count(&ndev) == SR_OK && ndev >= 0, "sr_device_count", 0);
  const bool gpu = ndev > 0;
  int rc;

  auto refused = [&](const std::string& what, const std::vector<uint8_t>& b) {
    write_file(path, b);
    const int r = load(path);
    expect(r == SR_ERR_IO, what, r);
  };

  for (int32_t dtype : {SR_DTYPE_F16, SR_DTYPE_FP8_E4M3}) {
    const std::string tag = dtype == SR_DTYPE_F16 ? "fp16: " : "fp8: ";
    const std::vector<uint8_t> v = snapshot(dtype);
    write_file(path, v);
    rc = load(path);
    expect(gpu ? rc == SR_OK : (rc != SR_OK && rc != SR_ERR_IO), tag + "valid snapshot parses", rc);
    for (size_t len = 0; len < v.size(); ++len)  // every truncation (0: the empty file)
      refused(tag + "truncated at " + std::to_string(len), std::vector<uint8_t>(v.begin(), v.begin() + len));
    {
      std::vector<uint8_t> ext = v;
      ext.push_back(0);
      refused(tag + "trailing byte", ext);
    }
    {
      std::vector<uint8_t> b = v;
      b[3] ^= 0x20;
      refused(tag + "bad magic", b);
    }
    for (int32_t d : {0, -64, 32, 96, 1088, 2048, 0x7fffffc0, (int32_t)0x80000000})
      refused(tag + "dim " + std::to_string(d), patched<int32_t>(v, 8, d));
    for (int32_t t : {0, 3, -1, 0x7fffffff, 256 + dtype})
      refused(tag + "dtype " + std::to_string(t), patched<int32_t>(v, 12, t));
    const int64_t big[] = {-1,
                           (int64_t(1) << 31) - 1,
                           int64_t(1) << 31,
                           int64_t(1) << 40,
                           (int64_t(1) << 40) + 1,
                           int64_t(1) << 62,
                           -(int64_t(1) << 62),
                           INT64_MIN,
                           INT64_MAX};
    for (int64_t x : big) {
      refused(tag + "n_rows " + std::to_string(x), patched<int64_t>(v, 16, x));
      refused(tag + "n_tokens " + std::to_string(x), patched<int64_t>(v, 24, x));
    }
    for (int64_t x : {kRows - 1, kRows + 1}) refused(tag + "n_rows " + std::to_string(x), patched<int64_t>(v, 16, x));
    for (int64_t x : {kTokens - 1, kTokens + 1})
      refused(tag + "n_tokens " + std::to_string(x), patched<int64_t>(v, 24, x));
    refused(tag + "off[0] != 0", patched<int64_t>(v, kOffAt, 1));
    refused(tag + "off[0] negative", patched<int64_t>(v, kOffAt, -1));
    refused(tag + "decreasing offset", patched<int64_t>(v, kOffAt + 8, kTokens + 1));
    refused(tag + "negative offset", patched<int64_t>(v, kOffAt + 16, -(int64_t(1) << 62)));
    refused(tag + "offset INT64_MIN", patched<int64_t>(v, kOffAt + 16, INT64_MIN));
    refused(tag + "off[n] != n_tokens", patched<int64_t>(v, kOffAt + 8 * kRows, kTokens + 1));
    refused(tag + "a row of 2^31 tokens",
            patched<int64_t>(patched<int64_t>(v, kOffAt + 8 * kRows, (int64_t(1) << 31) + 2), 24,
                             (int64_t(1) << 31) + 2));
    refused(tag + "live byte 2", patched<uint8_t>(v, kLiveAt, 2));
    refused(tag + "live byte 255", patched<uint8_t>(v, kLiveAt + 2, 255));
    if (dtype == SR_DTYPE_FP8_E4M3) {
      refused(tag + "fp8 byte 0x7f", patched<uint8_t>(v, kPoolAt + 5, 0x7f));
      refused(tag + "fp8 byte 0xff", patched<uint8_t>(v, v.size() - 1, 0xff));
    }
    // random bit flips in the header: never a crash, never a success without a device
    std::mt19937 rng(dtype == SR_DTYPE_F16 ? 1234 : 4321);
    for (int it = 0; it < 200; ++it) {
      std::vector<uint8_t> b = v;
      const int flips = 1 + (int)(rng() % 3);
      for (int f = 0; f < flips; ++f) b[rng() % 32] ^= (uint8_t)(1u << (rng() % 8));
      write_file(path, b);
      rc = load(path);
      expect(rc <= 0 && (gpu || rc != SR_OK), tag + "random header flip " + std::to_string(it), rc);
    }
  }
  rc = load(dir + "/does_not_exist.srmv");
  expect(rc == SR_ERR_IO, "missing file", rc);
  rc = load(dir);
  expect(rc == SR_ERR_IO, "a directory", rc);

  // ---- argument validation -------------------------------------------------------------------
  auto neg = [&](const std::string& what, int r) { expect(r < 0, what, r); };
  sr_mv* xn = nullptr;
  int64_t map[4];
  neg("mv_save(handle NULL)", sr_mv_save(nullptr, path.c_str()));
  neg("mv_save(both NULL)", sr_mv_save(nullptr, nullptr));
  neg("mv_load(path NULL)", sr_mv_load(nullptr, 0, &xn));
  neg("mv_load(out NULL)", sr_mv_load(path.c_str(), 0, nullptr));
  neg("mv_compact(handle NULL)", sr_mv_compact(nullptr, 0, map));
  neg("mv_compact(handle NULL, stage < 0)", sr_mv_compact(nullptr, -1, nullptr));
  neg("mv_compact(handle NULL, stage 1)", sr_mv_compact(nullptr, 1, nullptr));
  neg("mv_dim(NULL)", sr_mv_dim(nullptr, nullptr));
  if (gpu) {  // with a device: the checks behind a valid handle, which must leave the index as it was
    sr_mv* x = nullptr;
    rc = sr_mv_create(kDim, 0, &x);
    expect(rc == SR_OK && x, "mv_create", rc);
    if (x) {
      const int64_t off[3] = {0, 2, 3};
      std::vector<float> vecs(3 * kDim, 0.125f);
      const int64_t dead = 0;
      expect(sr_mv_add(x, off, vecs.data(), 2, nullptr) == SR_OK && sr_mv_remove(x, &dead, 1) == SR_OK, "mv_add", 0);
      neg("mv_save(path NULL)", sr_mv_save(x, nullptr));
      rc = sr_mv_save(x, (dir + "/no_such_dir/x.srmv").c_str());
      expect(rc == SR_ERR_IO, "mv_save(missing directory)", rc);
      for (int64_t sb : {int64_t(-1), int64_t(1), int64_t(2 * kDim - 1), INT64_MIN}) {
        rc = sr_mv_compact(x, sb, map);
        expect(rc == SR_ERR_INVALID, "mv_compact(stage_bytes " + std::to_string(sb) + ")", rc);
      }
      int64_t n = 0, live = 0, tok = 0;
      rc = sr_mv_stats(x, &n, &live, &tok);
      expect(rc == SR_OK && n == 2 && live == 1 && tok == 3, "mv_compact refusals left the index untouched", rc);
      rc = sr_mv_compact(x, 2 * kDim, map);
      expect(rc == SR_OK && map[0] == -1 && map[1] == 0, "mv_compact(one token of stage)", rc);
      sr_mv_destroy(x);
    }
  }
  expect(sr_last_error() != nullptr, "last_error after failures", 0);

  std::printf("fuzz_mv_loader: %d cases, %d failures (%s)\n", g_cases, g_fail,
              gpu ? "with a device" : "no device: parser and validation only");
  return g_fail ? 1 : 0;
}
