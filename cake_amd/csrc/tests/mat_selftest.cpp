// Host self-test of cake::Mat (csrc/engine/llama_weights.h): the sub-matrix offsets of every
// weight format, written out as literal byte counts, and the byte totals.  No GPU call: the
// Mats stand on fake base addresses that are never dereferenced.
// tests/test_engine_mat_cpu.py compiles and runs it.
#include <cstdint>
#include <cstdio>

#include "../engine/llama_weights.h"

namespace {

int failures = 0;

long long off(const void* p, const void* base) {
  return (long long)(reinterpret_cast<uintptr_t>(p) - reinterpret_cast<uintptr_t>(base));
}

void expect(const char* what, size_t r0, long long got, long long want) {
  if (got == want) return;
  std::fprintf(stderr, "FAIL %s at row %zu: %lld, expected %lld\n", what, r0, got, want);
  ++failures;
}

template <class T>
T* fake(uintptr_t a) {
  return reinterpret_cast<T*>(a);
}

struct Want {  // byte offsets of the sub-matrix from row r0 on, K = 2048
  size_t r0;
  long long w16, w8, scale, w4, e8, planes, hdr;
};

}  // namespace

int main() {
  using namespace cake;
  const size_t N = 6144, K = 2048;
  // q | k | v of 16 / 4 heads of 128 (rows 0, 4096, 5120) and gate | up (row N / 2)
  const Want want[] = {
      {0, 0, 0, 0, 0, 0, 0, 0},
      {4096, 16777216, 8388608, 16384, 4194304, 262144, 13631488, 16384},
      {5120, 20971520, 10485760, 20480, 5242880, 327680, 17039360, 20480},
      {3072, 12582912, 6291456, 12288, 3145728, 196608, 10223616, 12288},
  };
  Mat m16, m8, m4, mp;
  m16.N = m8.N = m4.N = mp.N = N;
  m16.K = m8.K = m4.K = mp.K = K;
  m16.w = fake<void>(0x10000000);
  m8.fmt = kFmtFp8;
  m8.w = fake<void>(0x20000000);
  m8.scale = fake<float>(0x28000000);
  m4.fmt = kFmtMxfp4;
  m4.w = fake<void>(0x30000000);
  m4.e8 = fake<uint8_t>(0x38000000);
  mp.w = fake<void>(0x40000000);  // 16-bit rows with a packed twin
  mp.p13.planes = fake<uint8_t>(0x50000000);
  mp.p13.hdr = fake<int>(0x58000000);
  mp.p13.raw = fake<uint16_t>(0x5c000000);

  for (const Want& x : want) {
    const Mat a = m16.rows(x.r0), b = m8.rows(x.r0), c = m4.rows(x.r0), d = mp.rows(x.r0);
    expect("16-bit rows", x.r0, off(a.w, m16.w), x.w16);
    expect("16-bit: no scales", x.r0, a.scale == nullptr && a.e8 == nullptr, 1);
    expect("16-bit: no twin", x.r0, a.p13.planes == nullptr && a.p13.hdr == nullptr, 1);
    expect("fp8 codes", x.r0, off(b.w, m8.w), x.w8);
    expect("fp8 row scales", x.r0, off(b.scale, m8.scale), x.scale);
    expect("fp8: no e8m0", x.r0, b.e8 == nullptr, 1);
    expect("mxfp4 codes", x.r0, off(c.w, m4.w), x.w4);
    expect("mxfp4 e8m0 bytes", x.r0, off(c.e8, m4.e8), x.e8);
    expect("mxfp4: no row scales", x.r0, c.scale == nullptr, 1);
    expect("packed twin: 16-bit rows", x.r0, off(d.w, mp.w), x.w16);
    expect("packed twin: planes", x.r0, off(d.p13.planes, mp.p13.planes), x.planes);
    expect("packed twin: headers", x.r0, off(d.p13.hdr, mp.p13.hdr), x.hdr);
    expect("packed twin: raw table unmoved", x.r0, off(d.p13.raw, mp.p13.raw), 0);
    for (const Mat* s : {&a, &b, &c, &d}) {
      expect("rows left", x.r0, (long long)s->N, (long long)(N - x.r0));
      expect("width", x.r0, (long long)s->K, (long long)K);
    }
    expect("format kept", x.r0, b.fmt == kFmtFp8 && c.fmt == kFmtMxfp4 && d.fmt == kFmt16, 1);
  }
  expect("rows(r0, n) row count", 4096, (long long)m8.rows(4096, 1024).N, 1024);
  expect("rows(r0, n) codes", 4096, off(m8.rows(4096, 1024).w, m8.w), 8388608);

  expect("16-bit bytes", 0, (long long)m16.bytes(), 25165824);           // N K 2
  expect("packed twin: 16-bit bytes", 0, (long long)mp.bytes(), 25165824);
  expect("fp8 bytes", 0, (long long)m8.bytes(), 12582912 + 24576);       // N K + 4 N
  expect("mxfp4 bytes", 0, (long long)m4.bytes(), 6291456 + 393216);     // N K / 2 + N K / 32

  expect("path 16-bit", 0, m16.path(), kPath16);
  expect("path fp8", 0, m8.path(), kPathW8);
  expect("path mxfp4", 0, m4.path(), kPathW4);
  expect("path packed twin", 0, mp.path(), kPathP13);
  expect("path of a packed sub-matrix", 4096, mp.rows(4096).path(), kPathP13);

  if (failures) return 1;
  std::printf("mat selftest ok\n");
  return 0;
}
