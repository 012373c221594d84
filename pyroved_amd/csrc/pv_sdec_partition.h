// pv_sdec_partition.h — the row partition every fused decoder kernel shares, its dL/d(hz) slots and the division-free walk over a
// workgroup's units: one text for the kernels, the host side (pv_sdec_fused_grid / pv_sdec_fused_kmax) and the test hook
// (pv_debug_partition_table / pv_debug_partition_walk in pv_sdec_fused.hip).  Plain integers in, plain integers out.
//
// The partition.  A UNIT is FD_UNIT = 16 rows of one decoder sample.  A sample occupies `rows` rows of the partition (its positions,
// or 16 ceil(positions / 16) in the tail form), upb = rows / 16 units; S samples (B, K B for a jiVAE, P B for P particles) make
// units = S upb.  G = min(max(units, 1), CUs) workgroups run; workgroup g owns the units [g units / G, (g + 1) units / G): every
// range holds at least one unit, and ranges differ by at most one.  A range whose length is 1 modulo the kernel's tile (4 or 8 units)
// ends in a column-parallel tail unit in the builds that have one.
// The slots.  Where a sample's rows end (or its own range does) a workgroup — in the bf16-class kernels each of its waves — publishes
// its partial dL/d(hz[b]) into sample b's slot (g - gfirst(b)) waves + wave, gfirst(b) = ceil((b upb + 1) G / units) - 1 being the
// workgroup that owns the sample's first unit, b upb.  A sample has kmax = (upb G / units + 2) waves slots: its upb units span
// upb G / units ranges of the average length units / G, plus a partial range at either end.  The bound has no slack — the last
// workgroup of a sample uses slot kmax - 1 in thousands of shapes and never a later one (tests/test_partition_cases_cpu.py) — so an
// off-by-one here writes into the next sample's slots: silent corruption, not a fault.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define FD_UNIT 16             // rows per unit: one wave's tile (one 16-column MFMA block)

#define SD_PART __host__ __device__ __forceinline__

SD_PART int sd_units_per_sample(int rows) { return rows / FD_UNIT; }

SD_PART int sd_grid(int64_t units, int cus) { return (int)(units < cus ? (units < 1 ? 1 : units) : cus); }

// workgroup g's range is [sd_unit_bound(g, ...), sd_unit_bound(g + 1, ...)); the 32-bit form where the launcher guarantees < 2^31 rows
SD_PART int64_t sd_unit_bound(int g, int64_t units, int G) { return (int64_t)g * units / G; }
SD_PART int sd_unit_bound32(int g, int64_t units, int G) { return (int)sd_unit_bound(g, units, G); }

template <class U>
SD_PART bool sd_ends_in_tail(U lo, U hi, int tile_units) { return ((hi - lo) & (tile_units - 1)) == 1; }

SD_PART int sd_gfirst(int b, int upb, int G, int64_t units) {
  const int64_t ub = (int64_t)b * upb;
  return (int)(((ub + 1) * G + units - 1) / units) - 1;
}

// WAVES: the waves that publish a slot each (1: the workgroup publishes one — the two f32 kernels, with wave = 0).  The four
// bf16-class kernels call sd_gfirst and write the last line out (under a comment that names this function): called from here, the
// compiler associates the sum in another order and their instructions move
template <int WAVES>
SD_PART int64_t sd_slot(int b, int g, int wave, int kmax, int upb, int G, int64_t units) {
  const int gfirst = sd_gfirst(b, upb, G, units);
  return (int64_t)b * kmax + (g - gfirst) * WAVES + wave;
}

SD_PART int sd_kmax(int rows, int64_t units, int grid, int waves) {
  const int64_t upb = sd_units_per_sample(rows);
  return ((int)((upb * grid) / (units > 0 ? units : 1)) + 2) * waves;
}

// ---- the walk: a unit's sample b, offset in the sample loc and observation unit xu, carried from tile to tile without a division
// (the int64 divisions this replaced expanded to ~900 scalar instructions per tile).  unit = b upb + loc ; xu = unit mod x_units where
// the observations repeat (x_units > 0: jiVAE, particles), else unit.  U: int below 2^31 rows, int64_t beyond
template <class U>
struct SdPos { U unit; int b, loc; U xu; };

template <class U>
SD_PART SdPos<U> sd_pos_of(U unit, int upb, U x_units) {
  SdPos<U> p;
  p.unit = unit; p.b = (int)(unit / upb); p.loc = (int)(unit - (U)p.b * upb);
  p.xu = x_units > 0 ? unit % x_units : unit;
  return p;
}

template <class U>
SD_PART void sd_pos_advance(SdPos<U>& p, int by, int upb, U x_units) {
  p.unit += by; p.loc += by; p.xu += by;
  while (p.loc >= upb) { p.loc -= upb; ++p.b; }
  if (x_units > 0) { while (p.xu >= x_units) p.xu -= x_units; }
}
