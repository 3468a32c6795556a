// gf_locate.h — the corrupted-shard locator (gf_locate.hip): a second use of
// the fused decode's check rows.
//
// For one erasure pattern, Q = the present shards in index order, S = the
// first k of them (the survivors), E = the remaining X = |Q| - k extras,
// C = G[E] x inv(G[S]) (X x k) and H = [C | I_X] over the columns S then E.
// s(c) = H x y(c) are the X syndromes of byte column c: exactly the check
// rows of build_reconstruct(..., check = true).  A single corrupted shard at
// column position q makes every s(c) a multiple of column q of H; with X >= 2
// and an MDS code no two columns are parallel, so the position is unique.
// Two entry points: one pattern for the whole batch (launch_locate), or one
// present mask per object read from HBM (launch_locate_masks, second half).
#pragma once
#include <cstdint>

#include <hip/hip_runtime_api.h>

#include "gf_apply.h"

namespace rsgpu {

constexpr int kLocMaxN = 16;  // shards of a code the locator serves
constexpr int kLocMinX = 2;   // extras: fewer cannot tell which shard is bad
constexpr int kLocMaxX = 4;
// per-object scratch word the locate kernel ORs into: bit q < k + X = column
// position q is dead (some byte column's syndromes are not parallel to it),
// kLocSeen = some syndrome byte is non-zero
constexpr uint32_t kLocSeen = 1u << 16;
constexpr int32_t kLocClean = -1, kLocUnlocatable = -2;  // RSGPU_LOC_*

// One erasure pattern's locator, host side (rsgpu.cpp build_locate)
struct LocPlan {
    int K = 0, X = 0;             // survivors, extras
    int nrows = 0;                // shards of the code (rows of an object)
    uint8_t order[kLocMaxN] = {}; // column position -> shard index (S then E)
    uint32_t present = 0;         // bit i: shard i present
    // [c][r][kCoefWords]: the table of C[r][c], as Pass::tab (input-major)
    uint32_t tab[(kLocMaxN - kLocMinX) * kLocMaxX * kCoefWords] = {};
};

// Locates on `stream`: acc (L.nobj u32) collects the dead-position masks: all
// zero and left zero (the status ring), or any words, loc itself included,
// with clear = true (a kernel zeroes them first).  The finish kernel writes
// loc[o] (kLocClean, kLocUnlocatable or the shard index) and, when masks !=
// nullptr, masks[o] = the present mask with the located shard cleared.
hipError_t launch_locate(const LocPlan &P, const Layout &L, uint32_t *acc, int32_t *loc, uint32_t *masks,
                         hipStream_t stream, bool clear = false);


// ---- per-object patterns (rsgpu_locate_dev_masks): the locator atlas
// Every pattern of the code the locator serves, as the kernels read it: a
// direct table over all 2^n present masks (a record slot, or the RSGPU_LOC_*
// code of a pattern that is not served), one LocRec per served pattern and
// the records' kernel tables.  Built per context from build_locate, one call
// per pattern, so the uniform and the masked calls share every byte of C.
constexpr int32_t kLocTooFew = -3, kLocTooMany = -4, kLocSingular = -5;  // RSGPU_LOC_*

struct alignas(16) LocRec {
    uint32_t X;           // extras (2..4)
    uint32_t pad;
    uint32_t order[2];    // nibble q: the shard at column position q (S then E), as LocPlan::order
    uint8_t coef[4][16];  // C[r][c], zero for r >= X or c >= k
};
static_assert(sizeof(LocRec) == 80, "LocRec layout (dword reads in the kernels)");

struct LocAtlasView {
    const int32_t *pat = nullptr;    // [1 << n]
    const LocRec *recs = nullptr;    // [slot]
    const uint32_t *tabs = nullptr;  // [slot][k][xmax][kCoefWords]: table of C[r][c], zero for r >= X
    const uint32_t *ctab = nullptr;  // [256][8] (the context's, as gf_apply_lanes)
    int n = 0, k = 0;
    int xmax = 2;                    // most extras of a served pattern: min(4, parity), at least 2
};

// Whether launch_locate_masks takes the short-row form for this layout: rows
// of <= 128 vectors, more than one object, and RSGPU_LOCATE_LANES != 0 (read
// once at load; 0 forces the long-row form, which is correct at any length).
bool locate_lanes_form(const Layout &L);

// Locates every object by its own pattern present[o] & ((1 << n) - 1).
//   long rows:  gf_locate_masked (gf_locate's body; mask, slot and record by
//               scalar loads) ORs into acc, gf_locate_finish_masked writes
//               loc / masks; acc and clear as launch_locate.
//   short rows: gf_locate_lanes, opw whole objects per workgroup, reduced per
//               object in LDS; acc is not used.
// loc[o]: shard index, kLocClean, kLocUnlocatable, or the table's code for a
// pattern that is not served (no row of that object is read).  masks
// (nullable, may be `present`): the n-bit mask with the located shard cleared.
hipError_t launch_locate_masks(const LocAtlasView &A, const Layout &L, const uint32_t *present, uint32_t *acc,
                               int32_t *loc, uint32_t *masks, hipStream_t stream, bool clear = false);

// Zeroes n words with a kernel on `stream`.  For stream captures: a replayed
// graph's memset nodes were seen not to have zeroed small counters before the
// kernels that follow them read them (tests/test_gpu_locate.py's graph test
// finds stale words), kernel-to-kernel order holds.
hipError_t launch_zero_u32(uint32_t *p, size_t n, hipStream_t stream);

}  // namespace rsgpu
