// How the two launches of a spherical-harmonic transform (sht.hip) are tiled: the field tile, the ring kernel's chunk and LDS bytes, both
// grids and the workspace, as one pure host function.  Plain C++17 - no HIP - so it can be asked without a GPU (anemoi_sht_plan in
// include/anemoi_hip.h, ops.sht_plan in Python, tests/test_sht_cpu.py).  sht.hip only launches what plan_sht returns.
//
// The two kernels of a direction:
//   ring kernel      one workgroup = (ring k, a tile of kShtRingThreads modes [forward] or points [inverse], a tile of `ft` fields).  It walks
//                    the ring's points (forward) or modes (inverse) in chunks of `chunk` elements staged in LDS, `ft` fields at a time.
//   Legendre kernel  one workgroup = leg_rows rows (degrees l [forward] or rings k [inverse]) x 64 modes x a tile of `ft` fields; no LDS.
//                    A thread owns 1 degree (forward) or 4 adjacent rings (inverse) of one mode; what it streams for a row (the ring spectra
//                    [f, :, m] forward, the coefficients [f, :, m] inverse) is loaded once for all of them.  Measured on the MI355X at O96
//                    with 80 fields: 4 rings per thread took the inverse from 279 to 205 us at truncation 191 and from 155 to
//                    114 us at truncation 95; 4 degrees per thread made the forward SLOWER (156 -> 288 us at truncation 95: a quarter of
//                    the waves, each a serial loop over the rings), so the forward keeps one.
//
// THE LDS BOUND.  The ring kernel stages ft * chunk values of 4 bytes (forward: real points) or 8 bytes (inverse: complex modes); chunk is
// sized so that this is at most kShtRingLdsBytes = 8 KiB whatever the ring length (20 points at the pole of every octahedral grid, 400 at
// O96's equator, 5 136 at O1280's): a longer ring takes more chunks, never more LDS.  8 KiB is 256 points or 128 modes of 8 fields per pass: a
// pass is then 256 x 8 loads against 256 x 256 x 16 FMAs per workgroup, so the two barriers around it are noise, a workgroup's LDS never
// limits the waves per CU, and O96 itself (400 points, 192 modes) already takes more than one pass, so the multi-pass path is the tested one.
// Twiddles are gathered from the per-ring table in global memory (a ring's table is at most 41 KB and is shared by every workgroup of the
// ring), so they do not count against it.
#pragma once
#include <stdint.h>

#include "anemoi_hip.h"

namespace anemoi {

void set_error(const char* fmt, ...);  // lib.cpp

constexpr int kShtRingThreads = 256;         // modes (forward) / points (inverse) per ring workgroup
constexpr int kShtLegFwdPerThread = 1;       // degrees a forward Legendre thread accumulates
constexpr int kShtLegInvPerThread = 4;       // rings an inverse Legendre thread accumulates: ft x 4 complex accumulators
constexpr int kShtLegWaves = 4;              // waves of 64 modes per Legendre workgroup
constexpr int kShtMaxFieldTile = 8;          // register accumulators per thread: 8 fields (16 floats where complex)
constexpr int kShtRingLdsBytes = 8 * 1024;   // the bound on the ring kernel's LDS

enum class ShtDir : int32_t { Forward = 0, Inverse = 1 };

struct ShtPlan {
  int ft = 0;                // fields per tile: 1, 2, 4 or 8 (a template argument of all four kernels)
  int chunk = 0;             // ring kernel: points (forward) / modes (inverse) staged per pass
  int lds_bytes = 0;         // ring kernel: ft * chunk * (4 | 8) <= kShtRingLdsBytes
  unsigned ring_grid[3] = {0, 0, 0};  // (rings, tiles of kShtRingThreads modes | points, field tiles)
  int leg_rows = 0;                   // Legendre kernel: degrees (forward) | rings (inverse) per workgroup
  unsigned leg_grid[3] = {0, 0, 0};   // (tiles of 64 modes, tiles of leg_rows degrees | rings, field tiles)
  int64_t workspace_bytes = 0;        // the ring spectra X / Y: [fields, rings, M] complex fp32
};

inline int sht_field_tile(int64_t n_fields) {
  int ft = 1;
  while (ft < kShtMaxFieldTile && ft < n_fields) ft *= 2;
  return ft;
}

// n_rings = K, max_ring = max n_k, truncation = M - 1 = L - 1.  Returns ANEMOI_OK or ANEMOI_E_INVALID (with the error text set).
inline int plan_sht(ShtDir dir, int64_t n_fields, int n_rings, int max_ring, int truncation, ShtPlan* out) {
  ShtPlan p;
  *out = p;
  if (n_rings <= 0 || max_ring <= 0) {
    set_error("sht: a grid of %d rings with at most %d points", n_rings, max_ring);
    return ANEMOI_E_INVALID;
  }
  if (truncation <= 0 || truncation > n_rings) {  // the reference's assertion (spectral_helpers.py:161-163)
    set_error("sht: truncation %d must be between 1 and the number of latitudes %d", truncation, n_rings);
    return ANEMOI_E_INVALID;
  }
  if (n_fields < 0 || n_fields >= (int64_t)1 << 24) {
    set_error("sht: %lld fields", (long long)n_fields);
    return ANEMOI_E_INVALID;
  }
  const int M = truncation + 1;
  p.ft = sht_field_tile(n_fields);
  const int elem = dir == ShtDir::Forward ? 4 : 8;
  const int extent = dir == ShtDir::Forward ? max_ring : (M < max_ring / 2 + 1 ? M : max_ring / 2 + 1);  // what a ring pass walks
  const int cap = kShtRingLdsBytes / (p.ft * elem);
  p.chunk = extent < cap ? extent : cap;
  p.lds_bytes = p.ft * p.chunk * elem;
  const unsigned ftiles = (unsigned)((n_fields + p.ft - 1) / p.ft);
  const int ring_items = dir == ShtDir::Forward ? M : max_ring;  // outputs of a ring: M modes (zero-filled past n_k/2) | n_k points
  p.ring_grid[0] = (unsigned)n_rings;
  p.ring_grid[1] = (unsigned)((ring_items + kShtRingThreads - 1) / kShtRingThreads);
  p.ring_grid[2] = ftiles;
  const int leg_rows = dir == ShtDir::Forward ? M : n_rings;
  p.leg_grid[0] = (unsigned)((M + 63) / 64);
  p.leg_rows = kShtLegWaves * (dir == ShtDir::Forward ? kShtLegFwdPerThread : kShtLegInvPerThread);
  p.leg_grid[1] = (unsigned)((leg_rows + p.leg_rows - 1) / p.leg_rows);
  p.leg_grid[2] = ftiles;
  p.workspace_bytes = n_fields * (int64_t)n_rings * M * 8;
  if (ftiles > 65535u || p.ring_grid[1] > 65535u || p.leg_grid[1] > 65535u) {
    set_error("sht: %lld fields / %d rings / truncation %d exceed the launch grid", (long long)n_fields, n_rings, truncation);
    return ANEMOI_E_INVALID;
  }
  *out = p;
  return ANEMOI_OK;
}

}  // namespace anemoi
