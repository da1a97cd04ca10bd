// slq_format.hpp — the formats an operator is stored in, as constants: the CSR pad, the caps of the workgroup tiles, the
// descriptor and record words of the ring-fed tile streams. Plain C++ (no HIP include): the kernels that read these formats
// (slq_kernels.hpp, slq_ring.hpp, slq_build.hpp, through slq_common.hpp) and the host code that writes them (slq_layout.hpp,
// which runs without a device) share this one file.
#pragma once
#include <stdint.h>

namespace slq {

// colind/vals of every stored CSR carry this many spare entries: the batched row gather (slq_kernels.hpp) loads indices and
// values 8 at a time and may read (never use) up to 7 entries past a row's end
constexpr int kCsrPad = 8;

// barrier tiles (k_csr_tile_pass, SLQ_TILES=1)
constexpr int kTileRows = 24;  // rows per tile at most (3 per wave)
constexpr int kTileCols = 72;  // distinct panel rows per tile at most: 72 KiB of LDS image

// ring-fed tiles (k_csr_ring_pass / k_ring_pass, SLQ_TILES=2)
#ifndef SLQ_RING_ROWS
#define SLQ_RING_ROWS 14
#endif
#ifndef SLQ_RING_COLS
#define SLQ_RING_COLS 36
#endif
constexpr int kRingTileRows = SLQ_RING_ROWS;  // two rows per consumer wave of a group
constexpr int kRingTileCols = SLQ_RING_COLS;  // distinct panel rows per tile at most
constexpr int kRingTileNnz = 112;             // nonzeros per tile at most: 128 B of header + 112 x (4 + 8) B fit 1.5 KiB (slq_ring.hpp: R merged tiles per slot)
constexpr int kRingMetaBytes = 2048;          // 4 slots x (36 + 2) KiB + kRingHeadBytes = 156 KiB
constexpr int kRingRecStride = 1536;          // bytes of record per base tile: 128 B of header + kRingTileNnz x (4 + 8)
// descriptor words (tile_desc[t * 64 + ...])
constexpr int kDescCols = 0, kDescRecOff = 1, kDescRecChunks = 2, kDescRow0 = 3, kDescRows = 4, kDescList = 8;
// The line list of an R = 1 descriptor is stored de-interleaved (r03): line d at word kDescList + ring1_list_pos(d), i.e. the
// even lines first, then the odd ones - the lines of each of TWO loader waves are then consecutive words, which a loader
// fetches with two wide scalar loads instead of eighteen single ones (slq_ring.hpp). Merged tiles (R > 1) keep line d at d.
constexpr int kRing1ListHalf = (kRingTileCols + 1) / 2;
#ifdef __HIPCC__
__host__ __device__
#endif
inline int ring1_list_pos(int d) { return (d & 1) * kRing1ListHalf + (d >> 1); }
// record words: [0 .. rows] row offsets into the record's own nonzeros, [15] byte offset of the values,
// [16 .. 16 + rows) line of each row's own panel row, then from byte 128 the column lines (int32) and the values (F)
constexpr int kRecValOff = 15, kRecSelf = 16, kRecHeadBytes = 128;

// ---- the constants a plan's shape is decided from (slq_plan_shape.hpp, which runs without a device), shared with the kernels ----
constexpr int kBlock = 512;          // threads per workgroup for the sweep kernels (8 waves)
constexpr int kWaves = kBlock / 64;
constexpr int kReorthChunk = 16;     // reorth columns whose dot accumulators live in registers
constexpr int kMaxDeg = 512;
constexpr int kMaxChebSteps = 16384;  // steps of a Chebyshev plan (2 * steps + 1 moments per probe; slq_cheb.hpp)
#ifndef SLQ_CHEB_ACC_COLS
#define SLQ_CHEB_ACC_COLS 16  // A/B builds (scripts/bench_cheb_action.py); the choice: DESIGN.md §4.13
#endif
// Finished ring columns one accumulation launch of a Chebyshev action plan consumes (k_cheb_accumulate; the plan's ring has as
// many slots): a launch moves (cols + 2) / cols panel passes per column. Bounded by the kernel's loads in flight: 4 VGPRs each.
constexpr int kChebAccCols = SLQ_CHEB_ACC_COLS;
static_assert(kChebAccCols >= 8 && kChebAccCols <= 16, "the live-column mask and the resident-workgroup budget of k_cheb_accumulate");
constexpr int kFusedMaxR = 8;        // fused recompute passes handle up to this many reorth columns
constexpr int kAccCols = 8;  // ring columns one accumulation launch consumes at most (their coefficients live in registers; slq_action.hpp)
constexpr int kDense32BM = 256, kDense32BN = 64, kDense32BK = 16, kDense32Pad = 32;  // k_dense_mfma32_lds: a workgroup's rows, columns, K stage, LDS row pad
#ifndef SLQ_TILE_DB
#define SLQ_TILE_DB 0  // k_csr_tile_pass: two tile images per workgroup
#endif

}  // namespace slq
