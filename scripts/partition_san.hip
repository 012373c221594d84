// partition_san.hip — pv_sdec_partition.h (the fused decoder kernels' row partition, its slots and the unit walk) under the host
// sanitizers: a stand-alone program, CPU only, nothing is launched and no device is needed.
//
//   SAN="-Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all -Xarch_host -g"
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -Ipyroved_amd/csrc $SAN -c scripts/partition_san.hip -o /tmp/partition_san.o
//   hipcc --offload-arch=gfx950 -fsanitize=address,undefined /tmp/partition_san.o -o /tmp/partition_san
//   /tmp/partition_san        prints the shapes walked and a checksum; a finding aborts, a wrong value returns its own status
//
// The shapes of tests/test_partition_cases_cpu.py (upb 1..19, 49, 64, 100, 256 x samples 1..699, 1024, 2048, 4096 on 256 compute units,
// and its six small shapes).  Per shape and per 1, 4 and 8 publishing waves every workgroup walks its range the way the kernels do —
// wave w from sd_pos_of(u_lo + w) by sd_pos_advance(waves), in 32- and in 64-bit units, with and without repeating observations — and marks the slot it would publish for
// each sample it meets in an array of exactly samples x kmax entries: every index is checked here before it is used, and the
// sanitizer watches the arrays' ends.
#include "pv_sdec_partition.h"
#include <stdio.h>
#include <vector>

template <int WAVES, class U>
static int walk_shape(int upb, int samples, int cus, bool every_period, unsigned long long& sum) {
  const int rows = upb * FD_UNIT;
  if (sd_units_per_sample(rows) != upb) return 2;
  const int64_t units = (int64_t)samples * upb;
  const int G = sd_grid(units, cus);
  const int kmax = sd_kmax(rows, units, G, WAVES);
  if (G < 1 || G > cus || G > units || kmax < 2 * WAVES) return 3;
  std::vector<unsigned char> seen((size_t)units, 0), slots((size_t)samples * kmax, 0);
  // observation periods: none, every sample its own (the jiVAE / particle form with one class / particle), a third of the samples
  std::vector<int64_t> periods = {0};
  if (every_period) periods = {0, units, (int64_t)upb * (samples / 3 > 0 ? samples / 3 : 1)};
  for (const int64_t x_units : periods) {
    for (auto& v : seen) v = 0;
    for (int g = 0; g < G; ++g) {
      const U lo = (U)sd_unit_bound(g, units, G), hi = (U)sd_unit_bound(g + 1, units, G);
      if ((int64_t)lo != sd_unit_bound32(g, units, G) || lo >= hi || (g == 0 && lo != 0) || (g == G - 1 && (int64_t)hi != units)) return 4;
      if (sd_ends_in_tail(lo, hi, 4) != ((hi - lo) % 4 == 1) || sd_ends_in_tail(lo, hi, 8) != ((hi - lo) % 8 == 1)) return 5;
      for (int w = 0; w < WAVES && lo + w < hi; ++w) {
        SdPos<U> p = sd_pos_of<U>(lo + w, upb, (U)x_units);
        for (;;) {
          if (p.unit < lo || p.unit >= hi || seen[(size_t)p.unit]) return 6;
          seen[(size_t)p.unit] = 1;
          if (p.b != (int)(p.unit / upb) || p.loc != (int)(p.unit % upb) || p.b < 0 || p.b >= samples) return 7;
          if ((int64_t)p.xu != (x_units > 0 ? (int64_t)p.unit % x_units : (int64_t)p.unit)) return 8;
          const int gfirst = sd_gfirst(p.b, upb, G, units);
          if (gfirst < 0 || gfirst > g || sd_unit_bound(gfirst, units, G) > (int64_t)p.b * upb ||
              sd_unit_bound(gfirst + 1, units, G) <= (int64_t)p.b * upb)
            return 9;                                     // gfirst owns the sample's first unit
          const int64_t slot = sd_slot<WAVES>(p.b, g, w, kmax, upb, G, units);
          if (slot < (int64_t)p.b * kmax || slot >= (int64_t)(p.b + 1) * kmax || slot >= (int64_t)slots.size()) return 10;
          slots[(size_t)slot] = 1;
          sum = sum * 1000003ull + (unsigned long long)slot + (unsigned long long)p.xu;
          if (p.unit + WAVES >= hi) break;
          sd_pos_advance(p, WAVES, upb, (U)x_units);
        }
      }
    }
    for (const auto v : seen)
      if (!v) return 11;
  }
  return 0;
}

static int shape(int upb, int samples, int cus, unsigned long long& sum) {
  // (the large shapes — up to a million units — take one period and two of the five forms: the run stays at seconds)
  const bool small = (int64_t)upb * samples <= 8192;
  int rc = walk_shape<8, int>(upb, samples, cus, small, sum);
  if (!rc) rc = walk_shape<4, int64_t>(upb, samples, cus, small, sum);
  if (!rc && small) rc = walk_shape<1, int64_t>(upb, samples, cus, true, sum);
  if (!rc && small) rc = walk_shape<4, int>(upb, samples, cus, true, sum);
  if (!rc && small) rc = walk_shape<8, int64_t>(upb, samples, cus, true, sum);
  if (rc) printf("upb %d samples %d cus %d: check %d failed\n", upb, samples, cus, rc);
  return rc;
}

int main() {
  unsigned long long sum = 0;
  long n = 0;
  std::vector<int> upbs, batches;
  for (int u = 1; u < 20; ++u) upbs.push_back(u);
  for (int u : {49, 64, 100, 256}) upbs.push_back(u);
  for (int b = 1; b < 700; ++b) batches.push_back(b);
  for (int b : {1024, 2048, 4096}) batches.push_back(b);
  for (int upb : upbs)
    for (int b : batches) {
      if (int rc = shape(upb, b, 256, sum)) return rc;
      ++n;
    }
  const int small[6][3] = {{1, 257, 256}, {3, 171, 256}, {49, 6, 256}, {4, 600, 256}, {1, 7, 4}, {2, 5, 3}};
  for (const auto& s : small) {
    if (int rc = shape(s[0], s[1], s[2], sum)) return rc;
    ++n;
  }
  printf("%ld shapes walked, checksum %llx\n", n, sum);
  return 0;
}
