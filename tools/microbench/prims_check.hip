// Checks the build primitives of csrc/lpa_prims.hip (radix sort, exclusive scans) and the shared
// edge-list builds of csrc/lpa_adj.hip against plain host references, at the sizes where their
// code changes path: around a wave (64), a block (256), a thread's vector (16) and a tile
// (lpa::kPrimTile elements), across scan levels, and past the grid cap of the block histograms.
//
//   prims_check scan | sort | adj      one group of cases; exit status 0 = every case matches
//
// Built by the csrc Makefile into build/lpa_hip/prims_check from lpa_prims.o and lpa_adj.o (the
// internals are reached by linking them; set_error is defined here), run on the GPU by
// tests/test_gpu_prims.py.  Every buffer the program hands to a primitive ends in 64 extra
// elements: 0xFF junk behind an input (a read past n changes the result), a 0xA5 pattern behind
// an output, checked afterwards (a write past the end is reported as a mismatch).
#include <stdarg.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <numeric>
#include <vector>

#include "lpa_device.h"
#include "lpa_algo.h"

namespace lpa {
static char g_err[512];
void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof g_err, fmt, ap);
  va_end(ap);
}
}  // namespace lpa

using lpa::u32;
using lpa::u64;
using lpa::ull;

namespace {

constexpr int64_t kPad = 64;       // junk / guard elements behind every buffer
constexpr int64_t kTile = lpa::kPrimTile;   // elements per block of the sort and the scans
static_assert(kTile == 4096, "the size lists below name 4079 .. 4097 and 8191 .. 8193 as tile edges: redo them");
constexpr uint8_t kJunk = 0xFF, kGuard = 0xA5;

hipStream_t g_s = nullptr;
const char* g_group = "?";
char g_case[256] = "(start)";
int64_t g_n = 0;
int g_cases = 0;

#define HIP_OK(call)                                                                                       \
  do {                                                                                                     \
    hipError_t e_ = (call);                                                                                \
    if (e_ != hipSuccess) {                                                                                \
      printf("prims_check %s: case '%s' n=%lld: %s failed: %s\n", g_group, g_case, (long long)g_n, #call, \
             hipGetErrorString(e_));                                                                       \
      fflush(stdout);                                                                                      \
      exit(2);                                                                                             \
    }                                                                                                      \
  } while (0)

#define LPA_OKAY(call)                                                                                        \
  do {                                                                                                        \
    int rc_ = (call);                                                                                         \
    if (rc_ != LPA_OK) {                                                                                      \
      printf("prims_check %s: case '%s' n=%lld: %s returned %d: %s\n", g_group, g_case, (long long)g_n, #call, \
             rc_, lpa::g_err);                                                                                \
      fflush(stdout);                                                                                         \
      exit(2);                                                                                                \
    }                                                                                                         \
  } while (0)

void begin_case(int64_t n, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_case, sizeof g_case, fmt, ap);
  va_end(ap);
  g_n = n;
}
// every case ends here: the stream is synchronised and its status checked
void end_case() {
  HIP_OK(hipStreamSynchronize(g_s));
  HIP_OK(hipGetLastError());
  ++g_cases;
}

[[noreturn]] void mismatch(const char* what, int64_t i, long long got, long long want) {
  printf("prims_check %s: MISMATCH case '%s' n=%lld: %s[%lld] = %lld (0x%llx), want %lld (0x%llx)\n", g_group, g_case,
         (long long)g_n, what, (long long)i, got, (unsigned long long)got, want, (unsigned long long)want);
  fflush(stdout);
  exit(1);
}
void check_eq(const char* what, long long got, long long want) {
  if (got != want) mismatch(what, 0, got, want);
}
template <typename T>
void compare(const char* what, const std::vector<T>& got, const std::vector<T>& want) {
  if (got.size() != want.size()) mismatch(what, -1, (long long)got.size(), (long long)want.size());
  if (got.empty() || memcmp(got.data(), want.data(), sizeof(T) * got.size()) == 0) return;
  size_t first = got.size(), last = 0, count = 0;
  for (size_t i = 0; i < got.size(); ++i)
    if (got[i] != want[i]) {
      if (count++ == 0) first = i;
      last = i;
    }
  printf("prims_check %s: %s differs at %zu of %zu elements, the last at index %zu\n", g_group, what, count, got.size(),
         last);
  mismatch(what, (int64_t)first, (long long)got[first], (long long)want[first]);
}

// splitmix64
struct Rng {
  u64 x;
  explicit Rng(u64 seed) : x(seed * 0x9E3779B97F4A7C15ull + 0x1234567ull) {}
  u64 next() {
    u64 z = (x += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
  }
  u64 below(u64 n) { return next() % n; }
};

// A device buffer of n elements at an allocation start (+ lead elements: the misaligned cases),
// followed by kPad elements; every byte starts as `fill`.
template <typename T>
struct Buf {
  T* base = nullptr;
  T* p = nullptr;
  int64_t n, lead;
  uint8_t fill;
  const char* name;
  Buf(const char* nm, int64_t n_, uint8_t fill_, int64_t lead_ = 0) : n(n_), lead(lead_), fill(fill_), name(nm) {
    LPA_OKAY(lpa::tmp_alloc((void**)&base, sizeof(T) * (size_t)(lead + n + kPad), g_s));
    HIP_OK(hipMemsetAsync(base, fill, sizeof(T) * (size_t)(lead + n + kPad), g_s));
    p = base + lead;
  }
  Buf(const char* nm, const std::vector<T>& h, uint8_t fill_, int64_t lead_ = 0) : Buf(nm, (int64_t)h.size(), fill_, lead_) {
    upload(h);
  }
  Buf(const Buf&) = delete;
  Buf& operator=(const Buf&) = delete;
  ~Buf() { lpa::tmp_free(base, g_s); }
  void upload(const std::vector<T>& h) {
    if (h.empty()) return;
    HIP_OK(hipMemcpyAsync(p, h.data(), sizeof(T) * h.size(), hipMemcpyHostToDevice, g_s));
    HIP_OK(hipStreamSynchronize(g_s));
  }
  // the n elements; the lead and the pad must still hold the fill pattern
  std::vector<T> fetch() {
    std::vector<T> all((size_t)(lead + n + kPad));
    HIP_OK(hipMemcpyAsync(all.data(), base, sizeof(T) * all.size(), hipMemcpyDeviceToHost, g_s));
    HIP_OK(hipStreamSynchronize(g_s));
    T pat;
    memset(&pat, fill, sizeof(T));
    char what[96];
    snprintf(what, sizeof what, "%s (guard, index from the buffer's start)", name);
    for (int64_t i = 0; i < lead; ++i)
      if (all[i] != pat) mismatch(what, i - lead, (long long)all[i], (long long)pat);
    for (int64_t i = lead + n; i < lead + n + kPad; ++i)
      if (all[i] != pat) mismatch(what, i - lead, (long long)all[i], (long long)pat);
    return std::vector<T>(all.begin() + lead, all.begin() + lead + n);
  }
};

template <typename T>
std::vector<T> d2h(const T* p, int64_t n) {
  std::vector<T> h((size_t)n);
  if (n > 0) HIP_OK(hipMemcpyAsync(h.data(), p, sizeof(T) * h.size(), hipMemcpyDeviceToHost, g_s));
  HIP_OK(hipStreamSynchronize(g_s));
  return h;
}

// ===========================================================================================
// scan
// ===========================================================================================
// out[i] = the sum of in[0, i), i in [0, n]: a 64-bit running sum, narrowed to Tout
template <typename Tin, typename Tout>
std::vector<Tout> scan_ref(const std::vector<Tin>& in) {
  std::vector<Tout> out(in.size() + 1);
  int64_t acc = 0;
  for (size_t i = 0; i < in.size(); ++i) {
    out[i] = (Tout)acc;
    acc += (int64_t)in[i];
  }
  out[in.size()] = (Tout)acc;
  return out;
}

template <typename Tin, typename Tout, typename F>
void scan_case(const std::vector<Tin>& in, F call, int64_t lead = 0) {
  const int64_t n = (int64_t)in.size();
  Buf<Tin> din("in", in, kJunk, lead);
  Buf<Tout> dout("out", n + 1, kGuard, lead);
  LPA_OKAY(call(din.p, dout.p, n, g_s));
  HIP_OK(hipStreamSynchronize(g_s));
  compare("out", dout.fetch(), scan_ref<Tin, Tout>(in));
  end_case();
}

void group_scan() {
  const int64_t sizes[] = {0,    1,    15,   16,   17,   63,   64,   65,   255,  256,           257,
                           4079, 4080, 4081, 4095, 4096, 4097, 8191, 8192, 8193, kTile * 17 + 5, kTile * kTile + 1};
  Rng rng(1);
  for (int64_t n : sizes) {
    // u8 -> u32
    for (int pat = 0; pat < 7; ++pat) {
      static const char* names[] = {"zeros", "ones", "half", "one at n-1", "one at 0", "bytes 0..255", "bytes 255"};
      std::vector<uint8_t> in((size_t)n);
      for (int64_t i = 0; i < n; ++i) {
        switch (pat) {
          case 0: in[i] = 0; break;
          case 1: in[i] = 1; break;
          case 2: in[i] = (uint8_t)(rng.next() >> 63); break;
          case 3: in[i] = i == n - 1; break;
          case 4: in[i] = i == 0; break;
          case 5: in[i] = (uint8_t)(rng.next() >> 56); break;   // total <= 255 n < 2^32 at every n here
          default: in[i] = 255; break;
        }
      }
      begin_case(n, "scan u8->u32 %s", names[pat]);
      scan_case<uint8_t, u32>(in, lpa::exclusive_scan_u8_u32);
      // in + 1 / out + 1: not 16-byte aligned, the generic form
      if (n == kTile * 17 + 5 || n == 4081 || n == 17) {
        begin_case(n, "scan u8->u32 %s, in + 1 and out + 1", names[pat]);
        scan_case<uint8_t, u32>(in, lpa::exclusive_scan_u8_u32, 1);
      }
    }
    // i32 -> i64
    for (int pat = 0; pat < 3; ++pat) {
      static const char* names[] = {"INT32_MAX", "signed mix", "small"};
      std::vector<int32_t> in((size_t)n);
      for (int64_t i = 0; i < n; ++i)
        in[i] = pat == 0 ? INT32_MAX : pat == 1 ? (int32_t)(u32)rng.next() : (int32_t)rng.below(3);
      begin_case(n, "scan i32->i64 %s", names[pat]);
      scan_case<int32_t, int64_t>(in, lpa::exclusive_scan_i32_i64);
    }
    // i64
    for (int pat = 0; pat < 2; ++pat) {
      static const char* names[] = {"above 2^32", "signed, above 2^32"};
      std::vector<int64_t> in((size_t)n);
      for (int64_t i = 0; i < n; ++i) {
        const int64_t v = (int64_t)(rng.next() >> 28) + (1ll << 32);   // [2^32, 2^32 + 2^36): |sum| < 2^62 at every n here
        in[i] = pat == 1 && (rng.next() & 1) ? -v : v;
      }
      begin_case(n, "scan i64 %s", names[pat]);
      scan_case<int64_t, int64_t>(in, lpa::exclusive_scan_i64);
    }
  }
}

// ===========================================================================================
// sort
// ===========================================================================================
enum Shape { SH_EQUAL, SH_WAVE64X4, SH_LANE, SH_ALT, SH_TILE, SH_RANDOM, SH_COUNT };
const char* kShapeNames[SH_COUNT] = {"all equal", "64 digits an item, all 256 over four items", "digit = lane", "alternating", "a tile a digit",
                                     "random"};

struct ShiftList {
  int shifts[8];
  int ns;
  int bits;        // the halves' sorted digits hold values of this many bits
  char name[32];
};

u64 digit_mask(const ShiftList& sl) {
  u64 m = 0;
  for (int i = 0; i < sl.ns; ++i) m |= 0xFFull << sl.shifts[i];
  return m;
}

// Keys for one case.  Every bit outside the sorted digits is random.  The first sorted digit
// follows the shape (by the key's index: what the first pass sees in its tiles, waves and
// lanes); the later ones are random, cut to the bits a half of `bits` bits has there.
std::vector<u64> make_keys(int64_t n, Shape shape, const ShiftList& sl, Rng& rng) {
  std::vector<u64> k((size_t)n);
  for (int64_t i = 0; i < n; ++i) {
    u64 x = rng.next();
    for (int j = 0; j < sl.ns; ++j) {
      const int sh = sl.shifts[j];
      const int have = sl.bits - (sh & 31);   // bits of the half's value inside this digit
      const u64 cut = have >= 8 ? 0xFFull : have <= 0 ? 0ull : (1ull << have) - 1ull;
      u64 dg = (x >> sh) & cut;
      if (j == 0) {
        const int64_t q = i % kTile;   // position in the tile: item q / 256, thread q % 256, lane q % 64
        switch (shape) {
          case SH_EQUAL: dg = 0x4D; break;
          case SH_WAVE64X4: dg = (u64)((64 * (q >> 8) + (q & 63)) & 255); break;
          case SH_LANE: dg = (u64)(q & 63); break;
          case SH_ALT: dg = (q & 1) ? 200 : 3; break;
          case SH_TILE: dg = (u64)(((i / kTile) * 37 + 5) & 255); break;
          default: break;
        }
      }
      x = (x & ~(0xFFull << sh)) | (dg << sh);
    }
    k[i] = x;
  }
  return k;
}

// the stable order of the keys by their sorted digits (the shift lists ascend: the masked key
// compares as the digit tuple does)
std::vector<u64> stable_perm(const std::vector<u64>& keys, u64 mask) {
  std::vector<u64> perm(keys.size());
  std::iota(perm.begin(), perm.end(), 0ull);
  std::stable_sort(perm.begin(), perm.end(), [&](u64 a, u64 b) { return (keys[a] & mask) < (keys[b] & mask); });
  return perm;
}

u64 payload_of(u64 i) { return i | (i << 32) | (1ull << 63); }   // the original index, in both halves

void sort_case(int64_t n, Shape shape, const ShiftList& sl, bool kv, Rng& rng) {
  begin_case(n, "%s %s, %s", kv ? "radix_sort_u64_kv" : "radix_sort_u64", sl.name, kShapeNames[shape]);
  const std::vector<u64> keys = make_keys(n, shape, sl, rng);
  const u64 mask = digit_mask(sl);
  std::vector<u64> want_k((size_t)n), want_v((size_t)n);
  if (sl.ns == 0 || n <= 1) {
    for (int64_t i = 0; i < n; ++i) want_k[i] = keys[i], want_v[i] = payload_of((u64)i);   // untouched
  } else if (!kv && n > (1 << 20)) {
    // the largest case: one stable sort of the keys themselves
    want_k = keys;
    std::stable_sort(want_k.begin(), want_k.end(), [mask](u64 a, u64 b) { return (a & mask) < (b & mask); });
  } else {
    const std::vector<u64> perm = stable_perm(keys, mask);
    for (int64_t i = 0; i < n; ++i) want_k[i] = keys[perm[i]], want_v[i] = payload_of(perm[i]);
  }
  Buf<u64> dk("keys", keys, kJunk);
  Buf<u64> dt("tmp keys", n, kGuard);
  if (!kv) {
    LPA_OKAY(lpa::radix_sort_u64(dk.p, dt.p, n, sl.shifts, sl.ns, g_s));
    HIP_OK(hipStreamSynchronize(g_s));
    compare("keys", dk.fetch(), want_k);
    const std::vector<u64> t = dt.fetch();   // the guard; untouched altogether on the early returns
    if (sl.ns == 0 || n <= 1) compare("tmp keys", t, std::vector<u64>((size_t)n, 0xA5A5A5A5A5A5A5A5ull));
  } else {
    std::vector<u64> vals((size_t)n);
    for (int64_t i = 0; i < n; ++i) vals[i] = payload_of((u64)i);
    Buf<u64> dv("vals", vals, kJunk);
    Buf<u64> dtv("tmp vals", n, kGuard);
    LPA_OKAY(lpa::radix_sort_u64_kv(dk.p, dv.p, dt.p, dtv.p, n, sl.shifts, sl.ns, g_s));
    HIP_OK(hipStreamSynchronize(g_s));
    compare("keys", dk.fetch(), want_k);
    compare("vals", dv.fetch(), want_v);
    const std::vector<u64> t = dt.fetch(), tv = dtv.fetch();
    if (sl.ns == 0 || n <= 1) {
      compare("tmp keys", t, std::vector<u64>((size_t)n, 0xA5A5A5A5A5A5A5A5ull));
      compare("tmp vals", tv, std::vector<u64>((size_t)n, 0xA5A5A5A5A5A5A5A5ull));
    }
  }
  end_case();
}

std::vector<ShiftList> shift_lists() {
  std::vector<ShiftList> out;
  const int bits[] = {1, 8, 9, 16, 17, 24, 25, 31};
  for (int b : bits) {
    const lpa::HalfShifts sh(b);
    for (int part = 0; part < 3; ++part) {
      ShiftList sl;
      sl.bits = b;
      sl.ns = part == 0 ? 2 * sh.ns : sh.ns;
      const int* src = part == 0 ? sh.both() : part == 1 ? sh.lo() : sh.hi();
      for (int i = 0; i < sl.ns; ++i) sl.shifts[i] = src[i];
      snprintf(sl.name, sizeof sl.name, "HalfShifts(%d).%s", b, part == 0 ? "both" : part == 1 ? "lo" : "hi");
      out.push_back(sl);
    }
  }
  ShiftList all_hi = {{32, 40, 48, 56}, 4, 32, "{32,40,48,56}"};   // lpa_pr.hip's all_hi; bit 63 set in half the keys
  out.push_back(all_hi);
  return out;
}

void group_sort() {
  Rng rng(2);
  const std::vector<ShiftList> lists = shift_lists();
  const int64_t sizes[] = {1, 2, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 8191, 8192, 8193, kTile * 17 + 1};
  for (int64_t n : sizes)
    for (const ShiftList& sl : lists)
      for (int shape = 0; shape < SH_COUNT; ++shape)
        for (int kv = 0; kv < 2; ++kv) sort_case(n, (Shape)shape, sl, kv != 0, rng);
  // the early returns: nothing to sort
  ShiftList none = {{0}, 0, 0, "no shifts"};
  for (int kv = 0; kv < 2; ++kv) {
    sort_case(100, SH_RANDOM, none, kv != 0, rng);
    sort_case(0, SH_RANDOM, lists[0], kv != 0, rng);
  }
  // more than 4096 tiles: the histogram (256 counters a tile) is scanned over two levels
  for (const ShiftList& sl : lists)
    if (!strcmp(sl.name, "HalfShifts(9).both")) sort_case((1ll << 24) + 1, SH_RANDOM, sl, false, rng);
}

// ===========================================================================================
// adj
// ===========================================================================================
struct Edges {
  std::vector<int32_t> s, d;
  void add(int64_t a, int64_t b) {
    s.push_back((int32_t)a);
    d.push_back((int32_t)b);
  }
};

// m edges over [0, V): duplicates, both directions of pairs, self-loops (0 and V - 1 among them),
// ids equal to V, above V and negative, and no edge at V / 2 (V >= 5).  pool: the vertices the
// random edges draw on (<= 0: every vertex)
Edges gen_edges(int64_t V, int64_t m, int64_t pool, Rng& rng) {
  Edges e;
  const int64_t iso = V >= 5 ? V / 2 : -1;
  std::vector<int64_t> pv;
  if (pool > 0 && pool < V) {
    for (int64_t i = 0; i < pool; ++i) {
      int64_t v = (int64_t)rng.below((u64)V);
      if (v == iso) v = 0;
      pv.push_back(v);
    }
  }
  auto vert = [&]() {
    int64_t v = pv.empty() ? (int64_t)rng.below((u64)V) : pv[rng.below(pv.size())];
    return v == iso ? V - 1 : v;
  };
  // the special edges first (as many as m admits), then random ones with duplicates and reversals
  const int64_t spec[][2] = {{0, V - 1},  {V - 1, 0}, {0, 0},        {V - 1, V - 1}, {V, 0},          {0, V},
                             {V, V},      {V + 7, 1}, {0, V + 100},  {-1, 0},        {0, -1},         {-5, -5},
                             {INT32_MIN, 0}, {INT32_MAX, INT32_MAX}, {0, V - 1},     {1 % V, 1 % V},  {V - 1, 0}};
  for (const auto& p : spec)
    if ((int64_t)e.s.size() < m) e.add(p[0], p[1]);
  while ((int64_t)e.s.size() < m) {
    const u64 r = rng.below(16);
    const size_t have = e.s.size();
    if (r == 0) {
      const size_t j = (size_t)rng.below(have);
      e.add(e.s[j], e.d[j]);   // a duplicate
    } else if (r == 1) {
      const size_t j = (size_t)rng.below(have);
      e.add(e.d[j], e.s[j]);   // the other direction
    } else if (r == 2) {
      const int64_t v = vert();
      e.add(v, v);
    } else if (r == 3) {
      e.add(vert(), V + (int64_t)rng.below(3));
    } else {
      e.add(vert(), vert());
    }
  }
  // shuffle
  for (size_t i = e.s.size(); i > 1; --i) {
    const size_t j = (size_t)rng.below(i);
    std::swap(e.s[i - 1], e.s[j]);
    std::swap(e.d[i - 1], e.d[j]);
  }
  return e;
}

struct AdjRef {
  std::vector<u64> akeys;                // every edge's (src << 32 | dst), or (V << 32 | V) when dropped, ascending
  std::vector<u64> arcs;                 // the distinct ones below (V << 32 | V)
  std::vector<int64_t> oo, io;
  std::vector<int32_t> ocol, icol;
  std::vector<uint8_t> loop;
  std::vector<u64> skeys;                // every edge's (min << 32 | max) or 0, ascending
  std::vector<int32_t> first;
  std::vector<int64_t> pos;
  std::vector<u64> simple;               // distinct (min << 32 | max), min != max, ascending
};

std::vector<int64_t> bounds_ref(const std::vector<u64>& keys, int64_t V, int shift) {
  std::vector<int64_t> out((size_t)V + 1);
  size_t i = 0;
  for (int64_t v = 0; v <= V; ++v) {
    while (i < keys.size() && (int64_t)(u32)(keys[i] >> shift) < v) ++i;
    out[v] = (int64_t)i;
  }
  return out;
}

void arcs_ref(int64_t V, const Edges& e, AdjRef* r) {
  const int64_t m = (int64_t)e.s.size();
  r->loop.assign((size_t)V, 0);
  const u64 dropped = ((u64)V << 32) | (u64)V;
  r->akeys.resize((size_t)m);
  for (int64_t i = 0; i < m; ++i) {
    const int64_t a = e.s[i], b = e.d[i];
    const bool in = a >= 0 && a < V && b >= 0 && b < V;
    if (in && a == b) r->loop[a] = 1;
    r->akeys[i] = in && a != b ? ((u64)a << 32) | (u64)b : dropped;
  }
  std::sort(r->akeys.begin(), r->akeys.end());
  r->arcs.clear();
  for (int64_t i = 0; i < m; ++i)
    if (r->akeys[i] != dropped && (i == 0 || r->akeys[i - 1] != r->akeys[i])) r->arcs.push_back(r->akeys[i]);
  const size_t E = r->arcs.size();
  r->oo = bounds_ref(r->arcs, V, 32);
  r->ocol.resize(E);
  std::vector<u64> t(E);
  for (size_t i = 0; i < E; ++i) {
    r->ocol[i] = (int32_t)(u32)r->arcs[i];
    t[i] = (r->arcs[i] << 32) | (r->arcs[i] >> 32);
  }
  std::sort(t.begin(), t.end());   // (dst, src): the sources ascend inside a row
  r->io = bounds_ref(t, V, 32);
  r->icol.resize(E);
  for (size_t i = 0; i < E; ++i) r->icol[i] = (int32_t)(u32)t[i];
}

void simple_ref(int64_t V, const Edges& e, AdjRef* r) {
  const int64_t m = (int64_t)e.s.size();
  r->skeys.resize((size_t)m);
  for (int64_t i = 0; i < m; ++i) {
    const int64_t a = e.s[i], b = e.d[i];
    const bool in = a >= 0 && a < V && b >= 0 && b < V;
    r->skeys[i] = in ? ((u64)std::min(a, b) << 32) | (u64)std::max(a, b) : 0ull;
  }
  std::sort(r->skeys.begin(), r->skeys.end());
  r->first.resize((size_t)m);
  r->pos.resize((size_t)m + 1);
  r->simple.clear();
  int64_t acc = 0;
  for (int64_t i = 0; i < m; ++i) {
    const u64 k = r->skeys[i];
    const bool f = (u32)(k >> 32) != (u32)k && (i == 0 || r->skeys[i - 1] != k);
    r->first[i] = f;
    r->pos[i] = acc;
    acc += f;
    if (f) r->simple.push_back(k);
  }
  r->pos[m] = acc;
}

lpa_graph* g_graph = nullptr;

// arcs_count + arcs_lists, loop given and null, and simple_edges on one edge list; want_arcs /
// want_simple >= 0: the case was built to have exactly that many distinct arcs / simple edges
void adj_case(int64_t V, const Edges& e, const char* what, int64_t want_arcs = -1, int64_t want_simple = -1) {
  const int64_t m = (int64_t)e.s.size();
  AdjRef r;
  Buf<int32_t> ds("e_src", e.s, kJunk), dd("e_dst", e.d, kJunk);
  lpa_graph* g = g_graph;
  g->V = V;
  g->m = m;
  g->e_src = ds.p;
  g->e_dst = dd.p;
  g->stream = g_s;

  arcs_ref(V, e, &r);
  if (want_arcs >= 0) check_eq("the reference's distinct arcs (the case's construction)", (long long)r.arcs.size(), want_arcs);
  for (int with_loop = 0; with_loop < 2; ++with_loop) {
    begin_case(m, "arcs V=%lld m=%lld %s, loop %s", (long long)V, (long long)m, what, with_loop ? "given" : "null");
    Buf<uint8_t> dl("loop", V, 0);   // zeroed by the caller; its pad is the guard
    lpa::Tmp tmp(g_s);
    lpa::ArcLists a;
    LPA_OKAY(lpa::arcs_count(g, tmp, with_loop ? dl.p : nullptr, &a));
    if (m > 0) {
      // between the steps: the sorted keys, a flag at the first of every arc, its scan
      compare("sorted keys", d2h(a.keys, m), r.akeys);
      std::vector<uint8_t> flag((size_t)m);
      std::vector<u32> pos((size_t)m + 1);
      u32 acc = 0;
      for (int64_t i = 0; i < m; ++i) {
        flag[i] = (int64_t)(r.akeys[i] >> 32) < V && (i == 0 || r.akeys[i - 1] != r.akeys[i]);
        pos[i] = acc;
        acc += flag[i];
      }
      pos[m] = acc;
      compare("flag", d2h(a.flag, m), flag);
      compare("pos", d2h(a.pos, m + 1), pos);
    }
    check_eq("E", (long long)a.E, (long long)r.arcs.size());
    LPA_OKAY(lpa::arcs_lists(g, tmp, &a));
    HIP_OK(hipStreamSynchronize(g_s));
    compare("oo", d2h(a.oo, V + 1), r.oo);
    compare("ocol", d2h(a.ocol, a.E), r.ocol);
    compare("io", d2h(a.io, V + 1), r.io);
    compare("icol", d2h(a.icol, a.E), r.icol);
    compare("loop", dl.fetch(), with_loop ? r.loop : std::vector<uint8_t>((size_t)V, 0));
    compare("e_src afterwards", ds.fetch(), e.s);   // the inputs and the junk behind them are as they were
    compare("e_dst afterwards", dd.fetch(), e.d);
    end_case();
  }

  begin_case(m, "simple_edges V=%lld m=%lld %s", (long long)V, (long long)m, what);
  simple_ref(V, e, &r);
  if (want_simple >= 0) check_eq("the reference's simple edges (the case's construction)", (long long)r.simple.size(), want_simple);
  {
    lpa::Tmp tmp(g_s);
    lpa::SimpleEdges se;
    LPA_OKAY(lpa::simple_edges(g, tmp, &se));
    HIP_OK(hipStreamSynchronize(g_s));
    check_eq("E", (long long)se.E, (long long)r.simple.size());
    if (m > 0) {
      const std::vector<u64> keys = d2h(se.keys, m);
      const std::vector<int32_t> first = d2h(se.first, m);
      compare("keys", keys, r.skeys);
      compare("first", first, r.first);
      compare("pos", d2h(se.pos, m + 1), r.pos);
      std::vector<u64> marked;
      for (int64_t i = 0; i < m; ++i)
        if (first[i]) marked.push_back(keys[i]);
      compare("keys with first set", marked, r.simple);
    }
    compare("e_src afterwards", ds.fetch(), e.s);
    compare("e_dst afterwards", dd.fetch(), e.d);
  }
  end_case();
}

// exactly 4096 distinct arcs u -> u + 1 + k (u, k in [0, 64)) and as many simple edges, + extra
// more; then duplicates, loops and out-of-range edges, and (reversed) the other directions, which
// add arcs but no simple edge
Edges exact_edges(int64_t V, int extra, bool reversed, Rng& rng) {
  Edges e;
  for (int u = 0; u < 64; ++u)
    for (int k = 0; k < 64; ++k) e.add(u, u + 1 + k);
  for (int x = 0; x < extra; ++x) e.add(200 + x, 230 + x);
  const size_t base = e.s.size();
  for (int i = 0; i < 1500; ++i) {
    const size_t j = (size_t)rng.below(base);
    const u64 r = rng.below(4);
    if (r == 0 && reversed) e.add(e.d[j], e.s[j]);
    else if (r == 1) e.add(e.s[j], e.s[j]);
    else if (r == 2) e.add(e.s[j], V + (int64_t)rng.below(2));
    else e.add(e.s[j], e.d[j]);
  }
  for (size_t i = e.s.size(); i > 1; --i) {
    const size_t j = (size_t)rng.below(i);
    std::swap(e.s[i - 1], e.s[j]);
    std::swap(e.d[i - 1], e.d[j]);
  }
  return e;
}

void bounds_cases(Rng& rng) {
  const int64_t Vs[] = {1, 257, 4097, 65537};
  const int64_t ns[] = {0, 1, 4095, 4096, 4097};
  for (int64_t V : Vs)
    for (int64_t n : ns)
      for (int high = 0; high < 2; ++high) {
        begin_case(n, "key_bounds / key_col V=%lld n=%lld %s half", (long long)V, (long long)n, high ? "high" : "low");
        // rows: none below V / 8 (the front), none in [V / 3, V / 2) (the middle), none from 3 V / 4 (the end)
        std::vector<u64> half((size_t)n);
        for (int64_t i = 0; i < n; ++i) {
          int64_t v;
          do v = (int64_t)rng.below((u64)V);
          while (V >= 16 && (v < V / 8 || (v >= V / 3 && v < V / 2) || v >= 3 * V / 4));
          half[i] = (u64)v;
        }
        std::sort(half.begin(), half.end());
        std::vector<u64> keys((size_t)n);
        std::vector<int32_t> col((size_t)n);
        for (int64_t i = 0; i < n; ++i) {
          const u64 other = rng.next() & 0xFFFFFFFFull;
          keys[i] = high ? (half[i] << 32) | other : (other << 32) | half[i];
          col[i] = (int32_t)(u32)keys[i];
        }
        Buf<u64> dk("keys", keys, kJunk);
        Buf<int64_t> dout("bounds", V + 1, kGuard);
        Buf<int32_t> dcol("col", n, kGuard);
        LPA_OKAY(lpa::key_bounds(dk.p, n, V, high != 0, dout.p, g_s));
        LPA_OKAY(lpa::key_col(dk.p, n, dcol.p, g_s));
        HIP_OK(hipStreamSynchronize(g_s));
        compare("bounds", dout.fetch(), bounds_ref(keys, V, high ? 32 : 0));
        compare("col", dcol.fetch(), col);
        end_case();
      }
}

void form_cases(Rng& rng) {
  const int64_t Vs[] = {1, 4095, 4096, 4097};
  const int64_t cuts[][2] = {{32, 1024}, {8, 1024}, {0, 16}, {32, 16}, {0, 0}};   // short_max, wave_max
  const char* mixes[] = {"all short", "all wave", "all block", "edges of the forms", "random"};
  for (int64_t V : Vs)
    for (const auto& c : cuts)
      for (int mix = 0; mix < 5; ++mix) {
        const int64_t sm = c[0], wm = c[1];
        begin_case(V, "form_lists V=%lld short_max=%lld wave_max=%lld %s", (long long)V, (long long)sm, (long long)wm,
                   mixes[mix]);
        const int64_t edge[] = {0, sm, sm + 1, wm, wm + 1};
        std::vector<int64_t> off((size_t)V + 1);
        std::vector<int32_t> wave, block;
        int64_t acc = 0;
        for (int64_t v = 0; v < V; ++v) {
          int64_t L;
          switch (mix) {
            case 0: L = (int64_t)rng.below((u64)sm + 1); break;
            case 1: L = wm > sm ? sm + 1 + (int64_t)rng.below((u64)(wm - sm)) : 0; break;
            case 2: L = std::max(sm, wm) + 1 + (int64_t)rng.below(5); break;
            case 3: L = edge[rng.below(5)]; break;
            default: L = rng.below(4) ? (int64_t)rng.below((u64)sm + 2) : (int64_t)rng.below(2 * (u64)wm + 40); break;
          }
          off[v] = acc;
          acc += L;
          if (L > sm && L <= wm) wave.push_back((int32_t)v);
          if (L > sm && L > wm) block.push_back((int32_t)v);
        }
        off[V] = acc;
        Buf<int64_t> doff("off", off, kJunk);
        lpa::Tmp tmp(g_s);
        int32_t* lists = nullptr;
        u32 n_rows[2] = {0xDEADu, 0xDEADu};
        LPA_OKAY(lpa::form_lists(tmp, doff.p, V, sm, wm, &lists, n_rows));
        HIP_OK(hipStreamSynchronize(g_s));   // n_rows is valid from here
        check_eq("n_rows[0]", n_rows[0], (long long)wave.size());
        check_eq("n_rows[1]", n_rows[1], (long long)block.size());
        compare("wave rows", d2h(lists, (int64_t)wave.size()), wave);
        compare("block rows", d2h(lists + V, (int64_t)block.size()), block);
        end_case();
      }
}

void comp_cases(Rng& rng) {
  const int64_t Vs[] = {1, 255, 256, 257, 4097, 256 * 2048 + 257};
  const char* kinds[] = {"one component", "singletons", "mix", "two tied for largest"};
  for (int64_t V : Vs)
    for (int kind = 0; kind < 4; ++kind) {
      if (kind == 3 && V < 2) continue;
      std::vector<int32_t> comp((size_t)V);
      if (kind == 0) {
        const int32_t r = (int32_t)(V / 3);
        for (int64_t v = 0; v < V; ++v) comp[v] = r;
      } else if (kind == 1) {
        for (int64_t v = 0; v < V; ++v) comp[v] = (int32_t)v;
      } else if (kind == 2) {
        // roots: about V / 16 vertices and vertex 0 (a giant: half the others join it)
        std::vector<int32_t> roots = {0};
        for (int64_t v = 1; v < V; ++v)
          if (rng.below(16) == 0) roots.push_back((int32_t)v);
        for (int64_t v = 0; v < V; ++v) comp[v] = rng.below(2) ? 0 : roots[rng.below(roots.size())];
        for (int32_t x : roots) comp[x] = x;
      } else {
        // halves of equal size under roots r1 < r2 (the summary names r1); an odd V leaves vertex
        // V - 1 a singleton
        const int64_t h = V / 2;
        const int32_t r1 = (int32_t)(h / 2), r2 = (int32_t)(h + h / 2);
        for (int64_t v = 0; v < 2 * h; ++v) comp[v] = v < h ? r1 : r2;
        if (V > 2 * h) comp[V - 1] = (int32_t)(V - 1);
      }
      std::vector<int64_t> size((size_t)V, 0);
      for (int64_t v = 0; v < V; ++v) size[comp[v]] += 1;
      ull want[3] = {0, 0, 0};
      for (int64_t v = 0; v < V; ++v)
        if (comp[v] == v) {
          want[0] += 1;
          want[1] += size[v] == 1;
          want[2] = std::max(want[2], ((ull)size[v] << 32) | (ull)(0xFFFFFFFFu - (u32)v));
        }
      for (int dev_out = 0; dev_out < 2; ++dev_out)
        for (int summary = 0; summary < 2; ++summary) {
          begin_case(V, "comp_sizes V=%lld %s, %s, %s", (long long)V, kinds[kind],
                     dev_out ? "size_out on the device" : "temporary sizes", summary ? "summary" : "no summary");
          Buf<int32_t> dc("comp", comp, kJunk);
          Buf<int64_t> dsz("size_out", V, kGuard);
          int64_t host_words[1] = {0};   // size_out on the host: not written by comp_sizes
          lpa::Tmp tmp(g_s);
          ull* size_dev = nullptr;
          ull h[3] = {~0ull, ~0ull, ~0ull};
          int64_t* size_out = dev_out ? dsz.p : summary ? host_words : nullptr;
          LPA_OKAY(lpa::comp_sizes(tmp, dc.p, V, size_out, dev_out, summary != 0, &size_dev, h));
          HIP_OK(hipStreamSynchronize(g_s));
          if (dev_out) check_eq("*size is size_out", (long long)(size_dev == (ull*)dsz.p), 1);
          compare("size", d2h((const int64_t*)size_dev, V), size);
          if (dev_out) compare("size_out", dsz.fetch(), size);
          else (void)dsz.fetch();
          check_eq("size_out on the host", host_words[0], 0);
          if (summary) {
            check_eq("components", (long long)h[0], (long long)want[0]);
            check_eq("singletons", (long long)h[1], (long long)want[1]);
            check_eq("largest (size << 32 | 0xFFFFFFFF - id)", (long long)h[2], (long long)want[2]);
          } else {
            check_eq("summary words untouched", (long long)(h[0] & h[1] & h[2]), -1ll);
          }
          end_case();
        }
    }
}

void group_adj() {
  Rng rng(3);
  g_graph = new lpa_graph();
  const int64_t Vs[] = {1, 2, 255, 256, 257, 65535, 65536, 65537};
  const int64_t ms[] = {0, 1, 4095, 4096, 4097, 8193};
  for (int64_t V : Vs)
    for (int64_t m : ms) {
      adj_case(V, gen_edges(V, m, V > 1000 ? 300 : 0, rng), "random, <= 300 vertices");
      if (V > 1000 && m > 1) adj_case(V, gen_edges(V, m, 0, rng), "random, every vertex");
    }
  // every edge a loop or out of range: E = 0 with m > 0 (arcs_lists clears its offsets)
  for (int64_t V : {1ll, 257ll, 65536ll}) {
    Edges e;
    for (int i = 0; i < 4097; ++i) {
      const int64_t v = (int64_t)rng.below((u64)V);
      if (i % 3 == 0) e.add(v, v);
      else if (i % 3 == 1) e.add(v, V + (int64_t)rng.below(2));
      else e.add(-1 - (int64_t)rng.below(5), v);
    }
    adj_case(V, e, "all dropped", 0, 0);
  }
  // the second sort, the compaction and the bounds search at a tile edge
  adj_case(257, exact_edges(257, 0, false, rng), "4096 distinct arcs", 4096, 4096);
  adj_case(65537, exact_edges(65537, 1, false, rng), "4097 distinct arcs", 4097, 4097);
  adj_case(65536, exact_edges(65536, 0, true, rng), "4096 simple edges, both directions", -1, 4096);
  adj_case(256, exact_edges(256, 1, true, rng), "4097 simple edges, both directions", -1, 4097);

  bounds_cases(rng);
  form_cases(rng);
  comp_cases(rng);
  delete g_graph;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2 || (strcmp(argv[1], "scan") && strcmp(argv[1], "sort") && strcmp(argv[1], "adj"))) {
    fprintf(stderr, "usage: prims_check scan|sort|adj\n");
    return 2;
  }
  g_group = argv[1];
  HIP_OK(hipSetDevice(0));
  HIP_OK(hipStreamCreate(&g_s));
  if (!strcmp(g_group, "scan")) group_scan();
  else if (!strcmp(g_group, "sort")) group_sort();
  else group_adj();
  HIP_OK(hipStreamSynchronize(g_s));
  HIP_OK(hipStreamDestroy(g_s));
  printf("prims_check %s: ok (%d cases)\n", g_group, g_cases);
  return 0;
}
