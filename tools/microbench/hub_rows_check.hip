// Checks the hub-row kernels that read a whole row per wave through the row-span loads of
// csrc/lpa_device.h (span_load, span_pair_batch) against plain host references, at the row
// lengths where the span loop changes path: one lane trip (64 elements), one span step
// (kSpanK x 64) and more, the settle's first words (kSettleK x 64) and its groups of four rows,
// the 64-row bounds batch and the grid-stride trip.
//
//   hub_rows_check settle | decide | code    one group of cases; exit status 0 = every case matches
//
//   settle   k_settle_big          rows of arc giant bits: rdirty, every udirty, Ln = G or untouched
//   decide   k_hub_decide          unit count sums, packed codes and plain: Ln, wcount, the listed
//                                  units and block-tier rows as sets, ndec
//   code     k_code_settle_hubs    the same sums: rdirty, every udirty, Ln
//
// Built by the csrc Makefile into build/lpa_hip/hub_rows_check from the library's objects (the
// internal launch wrappers of lpa_internal.h are reached by linking them), run on the GPU by
// tests/test_gpu_hub_rows.py.  Every input ends in junk (all ones: a read past the end changes a
// count), every output in a 0xA5 guard that is checked after each launch; each case is launched
// twice on the same buffers.
#include <stdarg.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "lpa_device.h"

using lpa::u32;
using lpa::u64;

namespace {

constexpr int64_t kPad = 64;  // junk / guard elements behind every buffer
constexpr int K = lpa::dev::kSpanK;
static_assert(K == 8, "the row lengths below name K x 4096 arcs and K x 64 units as 32768 and 512: redo them");
constexpr int32_t kG = 7, kSentinel = -77;
constexpr uint8_t kByteSentinel = 0x5A;

hipStream_t g_s = nullptr;
const char* g_group = "?";
char g_case[256] = "(start)";
int g_cases = 0;

#define HIP_OK(call)                                                                                        \
  do {                                                                                                      \
    hipError_t e_ = (call);                                                                                 \
    if (e_ != hipSuccess) {                                                                                 \
      printf("hub_rows_check %s: case '%s': %s failed: %s\n", g_group, g_case, #call, hipGetErrorString(e_)); \
      fflush(stdout);                                                                                       \
      exit(2);                                                                                              \
    }                                                                                                       \
  } while (0)
#define LPA_OKAY(call)                                                                          \
  do {                                                                                          \
    int rc_ = (call);                                                                           \
    if (rc_ != LPA_OK) {                                                                        \
      printf("hub_rows_check %s: case '%s': %s returned %d\n", g_group, g_case, #call, rc_);    \
      fflush(stdout);                                                                           \
      exit(2);                                                                                  \
    }                                                                                           \
  } while (0)

void begin_case(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_case, sizeof g_case, fmt, ap);
  va_end(ap);
}
void end_case() {
  HIP_OK(hipStreamSynchronize(g_s));
  HIP_OK(hipGetLastError());
  ++g_cases;
}
[[noreturn]] void mismatch(const char* what, int64_t row, int64_t i, long long got, long long want) {
  printf("hub_rows_check %s: MISMATCH case '%s': %s row %lld index %lld = %lld, want %lld\n", g_group, g_case, what,
         (long long)row, (long long)i, got, want);
  fflush(stdout);
  exit(1);
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

// n elements on the device followed by kPad elements, every byte of the pad `fill`
template <typename T>
struct Buf {
  T* p = nullptr;
  int64_t n;
  uint8_t fill;
  const char* name;
  Buf(const char* nm, int64_t n_, uint8_t fill_) : n(n_), fill(fill_), name(nm) {
    HIP_OK(hipMalloc((void**)&p, sizeof(T) * (size_t)(n + kPad)));
    HIP_OK(hipMemsetAsync(p, fill, sizeof(T) * (size_t)(n + kPad), g_s));
  }
  Buf(const char* nm, const std::vector<T>& h, uint8_t fill_) : Buf(nm, (int64_t)h.size(), fill_) {
    if (!h.empty()) HIP_OK(hipMemcpyAsync(p, h.data(), sizeof(T) * h.size(), hipMemcpyHostToDevice, g_s));
    HIP_OK(hipStreamSynchronize(g_s));
  }
  Buf(const Buf&) = delete;
  Buf& operator=(const Buf&) = delete;
  ~Buf() { (void)hipFree(p); }
  void set(const std::vector<T>& h) {
    if (!h.empty()) HIP_OK(hipMemcpyAsync(p, h.data(), sizeof(T) * h.size(), hipMemcpyHostToDevice, g_s));
    HIP_OK(hipStreamSynchronize(g_s));
  }
  // the n elements; the pad must still hold the fill pattern
  std::vector<T> fetch() {
    std::vector<T> all((size_t)(n + kPad));
    HIP_OK(hipMemcpyAsync(all.data(), p, sizeof(T) * all.size(), hipMemcpyDeviceToHost, g_s));
    HIP_OK(hipStreamSynchronize(g_s));
    T pat;
    memset(&pat, fill, sizeof(T));
    for (int64_t i = n; i < n + kPad; ++i)
      if (all[i] != pat) mismatch(name, -1, i, (long long)all[i], (long long)pat);
    all.resize((size_t)n);
    return all;
  }
};

std::vector<int32_t> gword_host(int g_try, int abits_ok, int code) {
  std::vector<int32_t> gw(64, 0);
  gw[lpa::GW_G] = kG;
  gw[lpa::GW_TRY] = g_try;
  gw[lpa::GW_ABITS_OK] = abits_ok;
  gw[lpa::GW_CODE] = code;
  return gw;
}

// ---------------------------------------------------------------------------
// settle: rows of consecutive arc ranges in one bit array
// ---------------------------------------------------------------------------
// set-bit patterns of a row of d arcs; every one with >= 2 set bits has the row's first
// and last bit set, so the bit just outside a neighbour is set and a mask that is off by
// one changes a count.  Rows take the patterns in this order, so a row with exactly half its
// bits set (not settled: the test is strict) lies between a row whose last word is full and a
// row that is all ones: one bit counted from either neighbour settles it wrongly.
// kFirstWord / kLastWord: half (even rows) or half + 1 (odd rows) of the bits, the row's first /
// last word filled before any other
enum Pat { kHalf, kAll, kHalfPlus, kNone, kRandom, kFirstWord, kLastWord, kPats };

struct SettleCase {
  std::vector<int64_t> rp, uoff;
  std::vector<u64> bits;
  std::vector<uint8_t> settled;  // host reference, per row
};

void set_bit(std::vector<u64>& w, int64_t i) { w[(size_t)(i >> 6)] |= 1ull << (i & 63); }
bool get_bit(const std::vector<u64>& w, int64_t i) { return (w[(size_t)(i >> 6)] >> (i & 63)) & 1ull; }

SettleCase make_settle(const std::vector<int64_t>& deg, int64_t off0, int pat0, u64 seed) {
  SettleCase c;
  Rng rng(seed);
  const int64_t n = (int64_t)deg.size();
  c.rp.assign((size_t)n + 1, off0);
  c.uoff.assign((size_t)n + 1, 0);
  for (int64_t v = 0; v < n; ++v) {
    c.rp[v + 1] = c.rp[v] + deg[v];
    c.uoff[v + 1] = c.uoff[v] + (deg[v] + lpa::kSegArcs - 1) / lpa::kSegArcs;
  }
  // the last row ends in the array's last word
  const int64_t end = c.rp[n], words = n ? (end + 63) / 64 : 1;
  c.bits.assign((size_t)words, 0ull);
  for (int64_t i = 0; i < off0; ++i) set_bit(c.bits, i);             // just below the first row
  for (int64_t i = end; i < words * 64 && n; ++i) set_bit(c.bits, i);  // just above the last one
  for (int64_t v = 0; v < n; ++v) {
    const int64_t a = c.rp[v], d = deg[v];
    const int pat = (int)((pat0 + v) % kPats);
    int64_t want = pat == kHalf ? d / 2 : pat == kHalfPlus ? d / 2 + 1 : pat == kAll ? d : pat == kNone ? 0
                 : pat == kRandom ? (int64_t)rng.below((u64)d + 1) : d / 2 + (int64_t)(v & 1);
    int64_t have = 0;
    auto put = [&](int64_t i) {
      if (!get_bit(c.bits, a + i)) {
        set_bit(c.bits, a + i);
        ++have;
      }
    };
    if (want >= 2) {
      put(0);
      put(d - 1);
    }
    if (pat == kFirstWord || pat == kLastWord) {
      // as many as fit of the set bits in the row's first / last word, the rest random
      const int64_t w_first_end = std::min<int64_t>(d, 64 - (a & 63));
      const int64_t w_last_beg = std::max<int64_t>(0, d - 1 - ((a + d - 1) & 63));
      if (pat == kFirstWord)
        for (int64_t i = 0; i < w_first_end && have < want; ++i) put(i);
      else
        for (int64_t i = d - 1; i >= w_last_beg && have < want; --i) put(i);
    }
    if (want == d) {
      for (int64_t i = 0; i < d; ++i) put(i);
    }
    while (have < want) put((int64_t)rng.below((u64)d));
  }
  c.settled.resize((size_t)n);
  for (int64_t v = 0; v < n; ++v) {
    int64_t cnt = 0;
    for (int64_t i = c.rp[v]; i < c.rp[v + 1]; ++i) cnt += get_bit(c.bits, i) ? 1 : 0;
    c.settled[v] = 2 * cnt > c.rp[v + 1] - c.rp[v] ? 1 : 0;
  }
  return c;
}

void run_settle(const SettleCase& c, int max_blocks, bool gate_fr_all = true, int gate_try = 1) {
  const int64_t n = (int64_t)c.rp.size() - 1, nu = c.uoff[n];
  Buf<int64_t> rp("rp", c.rp, 0xFF), uoff("uoff", c.uoff, 0xFF);
  Buf<u64> bits("abits", c.bits, 0xFF);
  Buf<int32_t> fr_all("fr_all", std::vector<int32_t>{gate_fr_all ? 1 : 0}, 0xA5);
  Buf<int32_t> gword("gword", gword_host(gate_try, 1, 0), 0xA5);
  Buf<int32_t> Ln("Ln", n, 0xA5);
  Buf<uint8_t> rd("rdirty", n, 0xA5), ud("udirty", nu, 0xA5);
  const bool on = gate_fr_all && gate_try;
  for (int round = 0; round < 2; ++round) {
    Ln.set(std::vector<int32_t>((size_t)n, kSentinel));
    rd.set(std::vector<uint8_t>((size_t)n, kByteSentinel));
    ud.set(std::vector<uint8_t>((size_t)nu, kByteSentinel));
    LPA_OKAY(lpa::launch_settle_big(g_s, rp.p, bits.p, n, fr_all.p, gword.p, Ln.p, rd.p, ud.p, uoff.p, max_blocks));
    HIP_OK(hipStreamSynchronize(g_s));
    const auto hL = Ln.fetch();
    const auto hr = rd.fetch();
    const auto hu = ud.fetch();
    (void)rp.fetch();
    (void)uoff.fetch();
    (void)bits.fetch();
    (void)gword.fetch();
    if (fr_all.fetch()[0] != (gate_fr_all ? 1 : 0)) mismatch("fr_all", -1, round, 0, 0);
    for (int64_t v = 0; v < n; ++v) {
      const int32_t wantL = on && c.settled[v] ? kG : kSentinel;
      const uint8_t wantd = on ? (c.settled[v] ? 0 : 1) : kByteSentinel;
      if (hL[v] != wantL) mismatch("Ln", v, round, hL[v], wantL);
      if (hr[v] != wantd) mismatch("rdirty", v, round, hr[v], wantd);
      for (int64_t u = c.uoff[v]; u < c.uoff[v + 1]; ++u)
        if (hu[u] != wantd) mismatch("udirty", v, u, hu[u], wantd);
    }
  }
  end_case();
}

// a row length that makes the row starting at bit `a` end on bit `endbit` of a word
int64_t deg_ending_at(int64_t a, int64_t base, int endbit) {
  int64_t d = base;
  while (((a + d - 1) & 63) != endbit) ++d;
  return d;
}

int group_settle() {
  // 16,384 arcs: the words k_settle_big issues with its rows in flight (kSettleK x 64), the span loop after
  const std::vector<int64_t> edges = {1025, 4095, 4096, 4097, 16383, 16384, 16385, (int64_t)K * 4096 - 1, (int64_t)K * 4096,
                                      (int64_t)K * 4096 + 1, 2 * (int64_t)K * 4096 - 1, 2 * (int64_t)K * 4096,
                                      2 * (int64_t)K * 4096 + 1, 4 * (int64_t)K * 4096 + 1};
  u64 seed = 1;
  for (int64_t off0 : {0, 1, 63}) {
    // every edge length with every pattern: kPats rounds, the pattern of row v is (r + v) % kPats
    for (int r = 0; r < kPats; ++r) {
      begin_case("edges off0=%lld pattern shift %d", (long long)off0, r);
      run_settle(make_settle(edges, off0, r, seed++), 0);
    }
    // rows ending on a word's last bit and on its first
    for (int endbit : {63, 0}) {
      std::vector<int64_t> deg;
      int64_t a = off0;
      for (int i = 0; i < (int)kPats; ++i) {
        deg.push_back(deg_ending_at(a, 1025 + 64 * i, endbit));
        a += deg.back();
      }
      begin_case("rows ending on bit %d of a word, off0=%lld", endbit, (long long)off0);
      run_settle(make_settle(deg, off0, 0, seed++), 0);
      begin_case("rows ending on bit %d of a word, off0=%lld, shifted patterns", endbit, (long long)off0);
      run_settle(make_settle(deg, off0, 1, seed++), 0);
    }
  }
  // the waves of a block, one more row than the grid's waves (max_blocks 2: 8 waves), and one
  // more than a wave's 64-row bounds batch holds (max_blocks 1: 4 waves x 64 rows)
  struct NH {
    int64_t n;
    int blocks;
  };
  for (NH t : {NH{0, 0}, NH{1, 0}, NH{3, 0}, NH{4, 0}, NH{5, 0}, NH{9, 2}, NH{257, 1}, NH{300, 1}}) {
    std::vector<int64_t> deg;
    Rng rng(100 + (u64)t.n);
    for (int64_t v = 0; v < t.n; ++v) deg.push_back(1025 + (int64_t)rng.below(200));
    begin_case("n_hub=%lld max_blocks=%d", (long long)t.n, t.blocks);
    run_settle(make_settle(deg, 5, (int)(t.n % kPats), seed++), t.blocks);
  }
  // the gate closed: nothing may be written
  begin_case("gate: fr_all = 0");
  run_settle(make_settle(edges, 1, 0, seed++), 0, false, 1);
  begin_case("gate: GW_TRY = 0");
  run_settle(make_settle(edges, 1, 0, seed++), 0, true, 0);
  return 0;
}

// ---------------------------------------------------------------------------
// decide / code: per-unit counts of consecutive unit ranges
// ---------------------------------------------------------------------------
struct UnitCase {
  std::vector<int64_t> uoff;
  std::vector<uint32_t> ugc, umx;
  std::vector<uint8_t> settled;
};

// row modes: sg == the bound (strict test: not settled) or the bound + 1 (settled), reached by one
// adjusted unit with a large G count, the row's first or its last, and random counts.  Every other
// unit has ugc <= 50 < 100 <= each umx count, so a unit dropped or counted twice at either end
// flips one of the four engineered modes
constexpr int kModes = 5;
UnitCase make_units(const std::vector<int>& nus, bool code, int mode0, u64 seed) {
  UnitCase c;
  Rng rng(seed);
  const int64_t n = (int64_t)nus.size();
  c.uoff.assign((size_t)n + 1, 0);
  for (int64_t h = 0; h < n; ++h) c.uoff[h + 1] = c.uoff[h] + nus[h];
  c.ugc.resize((size_t)c.uoff[n]);
  c.umx.resize((size_t)c.uoff[n]);
  c.settled.resize((size_t)n);
  for (int64_t h = 0; h < n; ++h) {
    const int64_t u0 = c.uoff[h], u1 = c.uoff[h + 1];
    u64 sg = 0, sm = 0, s1 = 0, s2 = 0, s3 = 0;
    for (int64_t u = u0; u < u1; ++u) {
      c.ugc[u] = (uint32_t)rng.below(51);
      if (code) {
        const u32 f1 = 100 + (u32)rng.below(241), f2 = 100 + (u32)rng.below(241), f3 = 100 + (u32)rng.below(241);
        c.umx[u] = f1 | (f2 << 10) | (f3 << 20);
        s1 += f1;
        s2 += f2;
        s3 += f3;
      } else {
        c.umx[u] = 100 + (u32)rng.below(413);
        sm += c.umx[u];
      }
      sg += c.ugc[u];
    }
    if (code) sm = std::max(s1, std::max(s2, s3));
    const int mode = (int)((mode0 + h) % kModes);   // 0 tie / first, 1 tie + 1 / last, 2 tie / last, 3 tie + 1 / first
    if (mode < 4 && u1 > u0) {
      const int64_t u = (mode == 0 || mode == 3) ? u0 : u1 - 1;
      sg -= c.ugc[u];
      c.ugc[u] = (uint32_t)(sm - sg + (u64)(mode & 1));  // sm >= 100 nu > sg
      sg += c.ugc[u];
    }
    c.settled[h] = sg > sm ? 1 : 0;
  }
  return c;
}

// wave rows [0, hb2) with the unit counts `wave_nus`, then lane rows (<= 16 units)
void run_decide(const std::vector<int>& wave_nus, int n_lane, bool code, int mode0, int max_blocks, int g_try, u64 seed) {
  std::vector<int> nus = wave_nus;
  Rng rng(seed ^ 0xABCDull);
  for (int i = 0; i < n_lane; ++i) nus.push_back(i < 15 ? 2 + i : 2 + (int)rng.below(15));
  const UnitCase c = make_units(nus, code, mode0, seed);
  const int64_t n = (int64_t)nus.size(), hb2 = (int64_t)wave_nus.size(), nu = c.uoff[n];
  Buf<int64_t> uoff("uoff", c.uoff, 0xFF);
  Buf<uint32_t> ugc("ugc", c.ugc, 0xFF), umx("umx", c.umx, 0xFF);
  Buf<int32_t> gword("gword", gword_host(g_try, 0, code ? 1 : 0), 0xA5);
  Buf<int32_t> Ln("Ln", n, 0xA5), wc("wcount", n, 0xA5), ul("ulist2", nu, 0xA5), gl("glist", n, 0xA5), nd("ndec", 4, 0xA5);
  for (int round = 0; round < 2; ++round) {
    Ln.set(std::vector<int32_t>((size_t)n, kSentinel));
    wc.set(std::vector<int32_t>((size_t)n, kSentinel));
    ul.set(std::vector<int32_t>((size_t)nu, kSentinel));
    gl.set(std::vector<int32_t>((size_t)n, kSentinel));
    nd.set(std::vector<int32_t>{0, 0, 0, kSentinel});
    LPA_OKAY(lpa::launch_hub_decide_rows(g_s, n, uoff.p, ugc.p, umx.p, gword.p, Ln.p, wc.p, ul.p, nd.p, hb2, gl.p,
                                         max_blocks));
    HIP_OK(hipStreamSynchronize(g_s));
    const auto hL = Ln.fetch(), hw = wc.fetch(), hnd = nd.fetch();
    auto hul = ul.fetch(), hgl = gl.fetch();
    (void)uoff.fetch();
    (void)ugc.fetch();
    (void)umx.fetch();
    (void)gword.fetch();
    if (hnd[lpa::GD_ALL] != (g_try ? 0 : 1)) mismatch("ndec[GD_ALL]", -1, round, hnd[lpa::GD_ALL], g_try ? 0 : 1);
    std::vector<int32_t> want_units, want_rows;
    for (int64_t h = 0; h < n; ++h) {
      const bool st = g_try && c.settled[h];
      const int32_t wantL = st ? kG : kSentinel;
      const int32_t wantw = !g_try || h >= hb2 ? kSentinel : st ? -1 : 0;
      if (hL[h] != wantL) mismatch("Ln", h, round, hL[h], wantL);
      if (hw[h] != wantw) mismatch("wcount", h, round, hw[h], wantw);
      if (g_try && !st) {
        if (h < hb2)
          for (int64_t u = c.uoff[h]; u < c.uoff[h + 1]; ++u) want_units.push_back((int32_t)u);
        else
          want_rows.push_back((int32_t)h);
      }
    }
    if (hnd[lpa::GD_UNITS] != (int32_t)want_units.size())
      mismatch("ndec[GD_UNITS]", -1, round, hnd[lpa::GD_UNITS], (long long)want_units.size());
    if (hnd[lpa::GD_ROWS] != (int32_t)want_rows.size())
      mismatch("ndec[GD_ROWS]", -1, round, hnd[lpa::GD_ROWS], (long long)want_rows.size());
    std::sort(hul.begin(), hul.begin() + (int64_t)want_units.size());
    std::sort(hgl.begin(), hgl.begin() + (int64_t)want_rows.size());
    for (size_t i = 0; i < want_units.size(); ++i)
      if (hul[i] != want_units[i]) mismatch("ulist2 (sorted)", -1, (int64_t)i, hul[i], want_units[i]);
    for (size_t i = want_units.size(); i < hul.size(); ++i)
      if (hul[i] != kSentinel) mismatch("ulist2 past its count", -1, (int64_t)i, hul[i], kSentinel);
    for (size_t i = 0; i < want_rows.size(); ++i)
      if (hgl[i] != want_rows[i]) mismatch("glist (sorted)", -1, (int64_t)i, hgl[i], want_rows[i]);
    for (size_t i = want_rows.size(); i < hgl.size(); ++i)
      if (hgl[i] != kSentinel) mismatch("glist past its count", -1, (int64_t)i, hgl[i], kSentinel);
  }
  end_case();
}

// unit counts around a lane trip (64), a span step (K x 64) and two steps; 2 is the shortest hub row
const std::vector<int> kUnitEdges = {2, 17, 63, 64, 65, K * 64 - 1, K * 64, K * 64 + 1, 2 * K * 64 - 1,
                                     2 * K * 64, 2 * K * 64 + 1, 1444};

int group_decide() {
  u64 seed = 1000;
  for (int code = 0; code < 2; ++code)
    for (int m = 0; m < kModes; ++m) {
      begin_case("unit edges code=%d mode shift %d, 40 lane rows", code, m);
      run_decide(kUnitEdges, 40, code != 0, m, 0, 1, seed++);
    }
  struct NH {
    int n_wave, n_lane, blocks;
  };
  for (NH t : {NH{1, 0, 0}, NH{3, 0, 0}, NH{4, 1, 0}, NH{5, 0, 0}, NH{0, 5, 0}, NH{9, 3, 2}, NH{257, 257, 1},
               NH{0, 513, 2}}) {
    std::vector<int> nus;
    Rng rng(200 + (u64)t.n_wave);
    for (int i = 0; i < t.n_wave; ++i) nus.push_back(17 + (int)rng.below(100));
    for (int code = 0; code < 2; ++code) {
      begin_case("wave rows=%d lane rows=%d max_blocks=%d code=%d", t.n_wave, t.n_lane, t.blocks, code);
      run_decide(nus, t.n_lane, code != 0, t.n_wave % kModes, t.blocks, 1, seed++);
    }
  }
  begin_case("gate: GW_TRY = 0");
  run_decide(kUnitEdges, 40, true, 0, 0, 0, seed++);
  return 0;
}

void run_code(const std::vector<int>& nus, int mode0, int max_blocks, int code_on, u64 seed) {
  const UnitCase c = make_units(nus, true, mode0, seed);
  const int64_t n = (int64_t)nus.size(), nu = c.uoff[n];
  Buf<int64_t> uoff("uoff", c.uoff, 0xFF);
  Buf<uint32_t> ugc("ugc", c.ugc, 0xFF), umx("umx", c.umx, 0xFF);
  Buf<int32_t> gword("gword", gword_host(1, 0, code_on), 0xA5);
  Buf<int32_t> Ln("Ln", n, 0xA5);
  Buf<uint8_t> rd("rdirty", n, 0xA5), ud("udirty", nu, 0xA5);
  for (int round = 0; round < 2; ++round) {
    Ln.set(std::vector<int32_t>((size_t)n, kSentinel));
    rd.set(std::vector<uint8_t>((size_t)n, kByteSentinel));
    ud.set(std::vector<uint8_t>((size_t)nu, kByteSentinel));
    LPA_OKAY(lpa::launch_code_settle_hubs(g_s, uoff.p, ugc.p, umx.p, n, gword.p, Ln.p, rd.p, ud.p, max_blocks));
    HIP_OK(hipStreamSynchronize(g_s));
    const auto hL = Ln.fetch();
    const auto hr = rd.fetch();
    const auto hu = ud.fetch();
    (void)uoff.fetch();
    (void)ugc.fetch();
    (void)umx.fetch();
    (void)gword.fetch();
    for (int64_t h = 0; h < n; ++h) {
      const int32_t wantL = code_on && c.settled[h] ? kG : kSentinel;
      const uint8_t wantd = code_on ? (c.settled[h] ? 0 : 1) : kByteSentinel;
      if (hL[h] != wantL) mismatch("Ln", h, round, hL[h], wantL);
      if (hr[h] != wantd) mismatch("rdirty", h, round, hr[h], wantd);
      for (int64_t u = c.uoff[h]; u < c.uoff[h + 1]; ++u)
        if (hu[u] != wantd) mismatch("udirty", h, u, hu[u], wantd);
    }
  }
  end_case();
}

int group_code() {
  u64 seed = 2000;
  for (int m = 0; m < kModes; ++m) {
    begin_case("unit edges mode shift %d", m);
    run_code(kUnitEdges, m, 0, 1, seed++);
  }
  struct NH {
    int n, blocks;
  };
  for (NH t : {NH{0, 0}, NH{1, 0}, NH{3, 0}, NH{4, 0}, NH{5, 0}, NH{9, 2}, NH{257, 1}, NH{300, 1}}) {
    std::vector<int> nus;
    Rng rng(300 + (u64)t.n);
    for (int i = 0; i < t.n; ++i) nus.push_back(2 + (int)rng.below(100));
    begin_case("n_hub=%d max_blocks=%d", t.n, t.blocks);
    run_code(nus, t.n % kModes, t.blocks, 1, seed++);
  }
  begin_case("gate: GW_CODE = 0");
  run_code(kUnitEdges, 0, 0, 0, seed++);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) {
    printf("usage: hub_rows_check settle|decide|code\n");
    return 2;
  }
  g_group = argv[1];
  HIP_OK(hipStreamCreate(&g_s));
  int rc = 2;
  if (!strcmp(argv[1], "settle")) rc = group_settle();
  else if (!strcmp(argv[1], "decide")) rc = group_decide();
  else if (!strcmp(argv[1], "code")) rc = group_code();
  else printf("hub_rows_check: unknown group '%s'\n", argv[1]);
  if (rc == 0) printf("hub_rows_check %s: ok (%d cases)\n", g_group, g_cases);
  fflush(stdout);
  return rc;
}
