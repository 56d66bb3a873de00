// bm_box_mfma.hip — the plain box matcher (bm_box.hip's semantics, bit-exact) with both window sums on the
// matrix pipe of gfx950: v_mfma_f32_16x16x32_f16 against banded 0/1 matrices.
//
// Scope: left view only (no fused right view), radius 1..kMaxFastRadius, valid_mode 0, d_max 64..256.
//
// Tile: 64 x 64 input pixels from (x0 - R, y0 - R) -> TOY x TOX outputs: 48 rows (three 16-row blocks; the
// fourth would be an edge block and its best keys the registers the paired loop needs) and 64 - 2R columns in
// NXB = 4 blocks (R = 7: 48 columns in 3).  A tile's d range is [d_lo, d_hi) cut on the right at W - x0 (no output of
// the tile has a larger valid d) and on the left one disparity past max(x_max + R + 1, d_lo), x_max the tile's last
// output column: from there on every window lies left of d, costs 0 and loses to that first one.  Four
// waves split the tile's d range and walk it two disparities per pass:
// one L read, two R reads, v_min3_u32 on the two keys of a pixel.  Each wave keeps its best keys for the whole
// tile in registers (12 * NXB VGPRs) in the accumulator layout, folded once at the end through LDS.  Ranges of at
// most 32 disparities at R <= 2 run the same loop with one d per pass on 64 - 2R rows (NP = 1, launch_rd).
// A workgroup walks a contiguous range of tiles; along a row of tiles it keeps the right band in LDS and stages
// only the new columns.  Large launches run one workgroup per resident slot, each drawing one run of
// tiles after another from a counter (box_mfma_queue_kernel).  The paired loop is written slot by slot,
// every MFMA between vector work of its own wave (run_paired), and carries its key constants and R
// addresses from pass to pass; a wave's masked passes are the same body plus the mask work, continuing
// where its unmasked passes end.  run() is the loop of the one-d-per-pass kernels alone.
//
// Exactness: every number is an integer its format holds exactly.
//   staging   L, R as f16 0x6400 | v = 1024 + v (unit spacing on [1024, 2048)): L' - R' == L - R exactly,
//             clearing the sign bits gives AD in 0..255.  Rows outside the image stage 0 on both sides (AD 0);
//             columns with c < d or c >= W get AD = 0 from the AND that clears the sign bits (a lane is one column),
//             and outputs with d > W - x start stage 2 from +inf, in the passes that have any.
//   stage 1   (vertical, M = 16 image columns, K = 32 input rows, N = 16 output rows)
//             D1 = sum AD - BIAS, BIAS = ceil((2R+1) * 255 / 2) in the C operand: |D1| <= 1913 < 2048 at R = 7,
//             so v_cvt_pk to f16 is exact.
//   stage 2   (horizontal, M = 16 output columns, K = 32 input columns, N = 16 output rows), band value 256,
//             C = 256 * (2R+1) * BIAS + d: the f32 accumulator is the key (S << 8 | d) < 2^24, and every partial
//             sum stays an integer below 2^24 in magnitude, so the accumulation order does not matter.
//   WTA       positive f32 bit patterns order like unsigned integers: min on the raw bits, ties to the smaller
//             d as in Device.cu:57 (the key's low byte is d, also within a pair); one v_cvt_u32_f32 per output
//             pixel in the epilogue, then the seed.
//
// Operand layout (lane l, g = l >> 4): A holds row l & 15, k = 8g..8g+7; B holds column l & 15, k = 8g..8g+7;
// C/D hold column l & 15, rows 4g..4g+3.  Stage 1's D (output row l & 15, image columns 4g..4g+3 of a
// 16-column block) packed to f16 is half of a stage-2 B operand; two adjacent column blocks make its K = 32 in
// the order (4g + j, 16 + 4g + j), and the constant horizontal band (the A operand) is built in that order.
// R sits in LDS column-major ([column][64 rows] f16, 128 B per column, 16-B row groups XOR-swizzled by the
// column), so a lane's R operand for any d is one ds_read_b128 at column x - d.  The rows of a column are permuted
// (staged_row): row group 4c + g holds the rows 32c + 4g + j and 32c + 16 + 4g + j, j = 0..3, so that a lane's eight
// AD registers hold, from register 2 ob on, the 32 input rows from the first row of output row block ob on, in that
// same K order.  The paired loop sums each row block with one MFMA on its four registers against one band (DESIGN
// §34); the one-d-per-pass loop multiplies the two chunks as read, the middle block from both.
#include <atomic>
#include <type_traits>

#include "bm_common.h"

namespace sm {
namespace {

typedef _Float16 h2 __attribute__((ext_vector_type(2)));
typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef float f4 __attribute__((ext_vector_type(4)));
typedef uint32_t u4 __attribute__((ext_vector_type(4)));
typedef uint32_t u8 __attribute__((ext_vector_type(8)));

constexpr int kT = 64;          // input tile edge
constexpr int kNW = 4;          // waves per workgroup, one per SIMD
constexpr int kThreads = 64 * kNW;
constexpr int kColB = 128;      // bytes per staged column (64 rows of f16)
constexpr uint32_t kInfBits = 0x7F800000u;
constexpr int kQueueLdsBytes = 16;   // behind a queue launch's staged tiles: the LDS word of the grab index

// NP: disparities per loop pass.  2: the paired loop on 48-row tiles.  1: one d per pass on 64 - 2R rows, for short
// d ranges at small radii, where a tile's staging and fold outweigh its loop and fewer, larger tiles win
template <int R, int DMAX, int NP>
struct MG {
    static_assert(NP == 1 || NP == 2, "one or two disparities per pass");
    // 16-row output blocks per tile: with two d per pass the fourth block's best keys are the registers the second
    // disparity needs
    static constexpr int NOB = NP == 2 ? 3 : 4;
    // 16-column output blocks per tile: four, the last one cut at 64 - 2R columns, while it keeps at least 4 columns;
    // at R = 7 (2 columns) three full blocks are faster (1080p D = 128, 32 frames: 1.376 against 1.421 ms)
    static constexpr int NXB = (NP == 1 || R <= 6) ? 4 : 3;
    static constexpr int TOY = NOB == 4 ? kT - 2 * R : 16 * NOB;   // output rows per tile
    static constexpr int TOX = NXB == 4 ? kT - 2 * R : 16 * NXB;   // output columns per tile
    static constexpr int FOLD = 16 * NXB + 1;                      // dwords per row of the fold plane
    static constexpr int RC = kT + DMAX;                           // staged right-band columns
    static constexpr int RS_BYTES = RC * kColB;
    static constexpr int L_BYTES = kT * kColB;
    static constexpr int LDS_BYTES = L_BYTES + RS_BYTES;           // the left tile first, then the right band
    static constexpr int BIAS = ((2 * R + 1) * 255 + 1) / 2;
    // A workgroup that goes on to the tile to the right keeps the RC - TOX band columns both tiles share: it moves
    // them down by TOX columns and stages the TOX new ones, as whole 4-column groups from column NEW0 on (the group
    // that straddles RC - TOX restages up to three moved columns with the values they already hold)
    static constexpr int KEEP = RC - TOX;
    static constexpr int NEW0 = KEEP & ~3;
    static constexpr int NEW4 = (RC - NEW0) / 4;                   // 4-column groups staged for a carried band
    static constexpr int MOVE_U = (KEEP * 8 + kThreads - 1) / kThreads;   // 16-B units per thread of the move
    static_assert(TOY + 2 * R <= kT && TOX + 2 * R <= kT, "every output's window lies in the input tile");
    static_assert(8 * NEW4 + 8 * (kT / 4) <= kThreads, "a carried tile stages in one pass");
    static_assert(TOY * FOLD * 4 <= L_BYTES + TOX * kColB,
                  "the fold plane aliases the left tile and the band columns the next tile drops, none it keeps");
    static_assert(BIAS < 2048 && (2 * R + 1) * 255 - BIAS < 2048, "D1 exact in f16");
    static_assert((int64_t)(2 * R + 1) * (2 * R + 1) * 255 * 256 + 255 < (1 << 24), "keys exact in f32");
};

// byte offset of 16-B row group q of staged column `col`
__device__ __forceinline__ int slot(int col, int q) { return col * kColB + ((q ^ ((col >> 1) & 7)) << 4); }

// The staged row that element i of row group q holds.  Group q = 4c + g is what lane group g reads of the 32-row
// chunk c: rows 32c + 4g + i (i < 4) and 32c + 16 + 4g + (i - 4) (i >= 4), the K order of a stage-2 operand.  A
// lane's two chunks are then eight registers in which the dwords 2 ob .. 2 ob + 3 hold the rows 16 ob + ko(g, j),
// ko = j < 4 ? 4g + j : 16 + 4g + (j - 4): the 32 input rows from output row block ob's first on
__device__ __forceinline__ constexpr int staged_row(int q, int i) {
    return 32 * (q >> 2) + 4 * (q & 3) + (i < 4 ? i : 12 + i);
}

// eight rows of one element (4 columns x 8 rows) as f16 1024 + v into columns `col`.. of row group q
__device__ __forceinline__ void stage_pack(const uint32_t (&w)[8], uint8_t* dst, int col, int q) {
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        u4 v;
#pragma unroll
        for (int m = 0; m < 4; ++m)
            v[m] = 0x64006400u | ((w[2 * m] >> (8 * b)) & 0xFFu) | (((w[2 * m + 1] >> (8 * b)) & 0xFFu) << 16);
        *reinterpret_cast<u4*>(dst + slot(col + b, q)) = v;
    }
}

// stage 4 * NC4 columns x 64 rows of `img` from (ytop, xleft), column-major
template <int NC4>
__device__ __forceinline__ void stage_cols(const uint8_t* img, int ytop, int xleft, int W, int H, int pitch,
                                           uint8_t* dst, int tid) {
    for (int e = tid; e < 8 * NC4; e += kThreads) {
        const int q = e / NC4, j = e - q * NC4;
        uint32_t w[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) w[i] = ld_image_u32(img, ytop + staged_row(q, i), xleft + 4 * j, W, H, pitch);
        stage_pack(w, dst, 4 * j, q);
    }
}

// A carried tile stages in one pass, one element per thread: the NEW4 new groups of the right band (from staged
// column NEW0) and the left tile.  Threads past the last element repeat it: no branch, the same bytes
template <int NEW0, int NEW4>
struct CarriedElem {
    bool right;
    int q, col, dx;   // row group, first staged column, image column offset from the piece's first
    __device__ __forceinline__ explicit CarriedElem(int tid) {
        constexpr int NR = 8 * NEW4, NL = 8 * (kT / 4);
        const int e = min(tid, NR + NL - 1);
        right = e < NR;
        const int el = e - NR;
        q = right ? e / NEW4 : el / (kT / 4);
        dx = 4 * (right ? e - q * NEW4 : el - q * (kT / 4));
        col = (right ? NEW0 : 0) + dx;
    }
};

// The thread index as a value the compiler takes to change from tile to tile: what staging and the band move derive
// from it (element indices, LDS slots) is then computed where it is used, not hoisted out of the tile loop and held
// in registers over the disparity loop, which has none to spare (no instruction is emitted)
__device__ __forceinline__ int per_tile(int tid) {
    asm volatile("" : "+v"(tid));
    return tid;
}

constexpr uint32_t kAbsBits = 0x7FFF7FFFu;

// |l - r| of eight staged pixels: v_pk_add_f16 with neg on r, then `keep` = kAbsBits clears the two sign bits; a
// lane whose image column is invalid passes keep = 0 and gets AD = 0 from the same AND
__device__ __forceinline__ u4 abs_diff(u4 l, u4 r, uint32_t keep) {
    u4 ad;
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const uint32_t lm = l[m], rm = r[m];
        const h2 d = __builtin_bit_cast(h2, lm) - __builtin_bit_cast(h2, rm);
        ad[m] = __builtin_bit_cast(uint32_t, d) & keep;
    }
    return ad;
}

__device__ __forceinline__ uint2 pack_f16(f4 v) {
    uint2 p;
    p.x = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_pkrtz(v[0], v[1]));   // exact: integers below 2048
    p.y = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_pkrtz(v[2], v[3]));
    return p;
}

__device__ __forceinline__ f4 mfma(u4 a, u4 b, f4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(h8, a), __builtin_bit_cast(h8, b), c, 0, 0, 0);
}

// The 32 input rows of output row block ob as a stage-1 A operand: dwords 2 ob .. 2 ob + 3 of a lane's eight AD
// registers (staged_row).  The vector passes through an empty asm first (no instruction is emitted): the three
// operands are then overlapping views of one 8-register tuple; left to itself the compiler splits the vector into
// three tuples and copies four registers per view
__device__ __forceinline__ u4 ad_view(u8& ad, int ob) {
    asm volatile("" : "+v"(ad));
    return ob == 0   ? __builtin_shufflevector(ad, ad, 0, 1, 2, 3)
           : ob == 1 ? __builtin_shufflevector(ad, ad, 2, 3, 4, 5)
                     : __builtin_shufflevector(ad, ad, 4, 5, 6, 7);
}

// WALK: the workgroup walks a range of tiles; false: one tile per workgroup, the tile loop and everything carried
// compiled away.  QUEUE (with WALK): the workgroup walks one run of tiles after another, box_queue_grab of what the
// launch's grab counter `queue`, zero at the launch, hands it; per is then the launch's tile count.  The
// kernels of static ranges are compiled without any of it
template <int R, int DMAX, int NP, bool WALK, bool QUEUE>
__device__ __forceinline__ void box_mfma_tiles(const MatchArgs& a, int tiles_x, int tiles_y, int per, int rem,
                                               uint32_t* queue) {
    using G = MG<R, DMAX, NP>;
    constexpr int NXB = G::NXB, NOB = G::NOB;
    // (aligned to 16 columns, the period of slot()'s swizzle in the address)
    extern __shared__ __attribute__((aligned(16 * kColB))) uint8_t smem[];
    uint8_t* lsm = smem;                  // [64][64] f16, swizzled
    uint8_t* rsm = smem + G::L_BYTES;     // [RC][64] f16, swizzled

    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lane = tid & 63;
    const int l16 = lane & 15;
    const int g = lane >> 4;

    // Workgroup position k of n walks the tiles [k T / n, (k + 1) T / n) of the sequence [frame][ty][tx]: with n = T
    // one tile each; with fewer, runs along a row of tiles, whose right bands overlap.  T = per n + rem from the
    // host, so k T / n = k per + k rem / n, and the 64-bit division is skipped where n divides T
    static_assert(!QUEUE || WALK, "a queue workgroup walks its runs");
    constexpr bool queued = QUEUE;
    const int wg = queued ? 0 : xcd_tile(blockIdx.x, gridDim.x);
    int t_begin = wg * per, t_end = t_begin + per;
    if (WALK && rem != 0) {
        t_begin += (int)((int64_t)wg * rem / (int)gridDim.x);
        t_end += (int)((int64_t)(wg + 1) * rem / (int)gridDim.x);
    }
    if constexpr (!WALK) t_end = t_begin + 1;
    // The queue: lane 0 of wave 0 draws, the grab index reaches the other waves through one LDS word behind the
    // staged tiles, which neither they nor the fold plane alias.  The word is written between a tile's first barrier
    // and the barrier after its disparity loops, and read after that one or, here, after a barrier of its own
    uint32_t* const qword = reinterpret_cast<uint32_t*>(smem + G::LDS_BYTES);
    auto take_run = [&] {
        const uint32_t gi = (uint32_t)__builtin_amdgcn_readfirstlane((int)*qword);
        const BoxGrab run = box_queue_grab(gi, (uint32_t)per, (uint32_t)tiles_x, gridDim.x);
        t_begin = (int)run.begin;
        t_end = (int)run.end;
    };
    if constexpr (queued) {
        if (tid == 0) *qword = atomicAdd(queue, 1u);
        __syncthreads();
        take_run();
    }
    if (t_begin >= t_end) return;
    const int tiles = tiles_x * tiles_y;
    int frame = t_begin / tiles;
    int ty = (t_begin - frame * tiles) / tiles_x;
    int tx = t_begin - frame * tiles - ty * tiles_x;
    const int W = a.W, H = a.H;
    const int d_lo = a.d_lo, d_hi = a.d_hi;

    // ---- constant bands ----
    // vertical (B operand of stage 1): a 32-row view of a lane's AD registers starts at its output row block's first
    // row (staged_row), so K slot (g, j) is input row ko = j < 4 ? 4g + j : 16 + 4g + (j - 4) of the block against
    // output row n = l16: 1.0 where 0 <= ko - n <= 2R, one band for every row block.  The one-d-per-pass loop (run())
    // multiplies the two chunks as they are read, rows 32c + ko, and needs two more: bv4, a chunk against the row
    // block 16 rows down (the middle block in chunk 0, the fourth in chunk 1): 1.0 where 0 <= ko - 16 - n <= 2R, and
    // bvp, chunk 1 against the middle block, 16 rows up: 1.0 where 0 <= ko + 16 - n <= 2R
    u4 bv, bv4, bvp;
    // horizontal (A operand of stage 2): 256.0 where 0 <= xin - l16 <= 2R; K = two 16-column blocks, elements
    // 0..3 of a lane the columns 4g.. of one and 4..7 of the other: bh with the left block first, bhs swapped
    u4 bh, bhs;
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        uint32_t wv = 0, w4 = 0, wp = 0, wh = 0, ws = 0;
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int j = 2 * m + e;
            const int xin = j < 4 ? 4 * g + j : 16 + 4 * g + (j - 4);   // ko as well
            const int dh = xin - l16;
            const int ds = (j < 4 ? 16 + 4 * g + j : 4 * g + (j - 4)) - l16;
            wv |= (dh >= 0 && dh <= 2 * R ? 0x3C00u : 0u) << (16 * e);
            w4 |= (dh - 16 >= 0 && dh - 16 <= 2 * R ? 0x3C00u : 0u) << (16 * e);
            wp |= (dh + 16 >= 0 && dh + 16 <= 2 * R ? 0x3C00u : 0u) << (16 * e);
            wh |= (dh >= 0 && dh <= 2 * R ? 0x5C00u : 0u) << (16 * e);
            ws |= (ds >= 0 && ds <= 2 * R ? 0x5C00u : 0u) << (16 * e);
        }
        bv[m] = wv;
        bv4[m] = w4;
        bvp[m] = wp;
        bh[m] = wh;
        bhs[m] = ws;
    }
    const float nbias = -(float)G::BIAS;
    const f4 c1 = {nbias, nbias, nbias, nbias};
    const float c2base = (float)(256 * (2 * R + 1) * G::BIAS);

    const int laddr = slot(l16, g);   // + 16 columns per block; chunk 1 is ^ 64

    bool carried = false;   // the tile's band and left tile are in LDS already (the end of the previous tile)
#pragma unroll 1
    for (int tile = t_begin;; ++tile) {
        const int x0 = tx * G::TOX;
        const int y0 = ty * G::TOY;
        const uint8_t* Lf = a.left + (int64_t)frame * a.frame_stride;
        const uint8_t* Rf = a.right + (int64_t)frame * a.frame_stride;

        // staged right column k is image column band0 + k: pixel column c at disparity d reads k = c - d - band0
        if (!carried) {
            const int band0 = x0 - R - d_lo - DMAX;
            const int st = per_tile(tid);
            stage_cols<G::RC / 4>(Rf, y0 - R, band0, W, H, a.pitch, rsm, st);
            stage_cols<kT / 4>(Lf, y0 - R, x0 - R, W, H, a.pitch, lsm, st);
        }

        // best keys as f32 bit patterns: [output row block][output column block][column 4g + i], row l16
        uint32_t best[NOB][NXB][4];
#pragma unroll
        for (int ob = 0; ob < NOB; ++ob)
#pragma unroll
            for (int xb = 0; xb < NXB; ++xb)
#pragma unroll
                for (int i = 0; i < 4; ++i) best[ob][xb][i] = kInfBits;

        // disparities past W - x0 are invalid for every output of the tile (Device.cu:44's break).  At the left edge
        // of the frame the range ends early as well (valid_mode 0 only, this file's scope): a staged
        // column c < d has AD = 0, so from d = x + R + 1 on the whole window of output column x lies left of d and
        // its key is (0 << 8) | d; in [d_lo, d_hi) the first such d, max(x + R + 1, d_lo), beats all later ones.
        // Past that disparity of its last output column x_max no key of the tile changes: that one pass still runs
        const int x_max = min(x0 + G::TOX, W) - 1;
        const int d_end = min(min(d_hi, W - x0 + 1), max(x_max + R + 1, d_lo) + 1);
        const int nd = max(d_end - d_lo, 0);
        const int dw_lo = d_lo + (wave * nd) / kNW;
        const int dw_hi = d_lo + ((wave + 1) * nd) / kNW;
        // largest d valid for every output of the tile
        const int d_free = W - x_max;
        // Both masks are monotone in d: a staged column c needs AD = 0 where c < d (from d = x0 - R + 1 on) or c >= W
        // (every d), an output column x has no key where d > W - x (from d = d_free + 1 on).  d_m is the first
        // disparity of the tile that needs either; each wave walks the whole passes below it in the unmasked loop and
        // the rest of its range in a masked one
        const int d_m = (x0 - R + kT > W) ? d_lo : max(min(x0 - R, d_free) + 1, d_lo);
        const int n_free = max(min(dw_hi, d_m) - dw_lo, 0);
        const int dw_m = dw_lo + n_free - n_free % NP;

        // Where the next tile of the range is the right-hand neighbour and its new band columns and left tile lie
        // inside the image (uniform per tile), its eight staging loads are unconditional dword loads, issued early
        // (issue_prefetch) and consumed after the fold
        const bool carry_next = WALK && tile + 1 < t_end && tx + 1 < tiles_x;
        const int nxl = x0 + G::TOX - R, nxr = nxl - d_lo - DMAX + G::NEW0;
        const bool prefetch = carry_next && y0 - R >= 0 && y0 - R + kT <= H && nxr >= 0 && nxl + kT <= W;
        uint32_t pw[8];
        auto issue_prefetch = [&] {
            if (prefetch) {
                const CarriedElem<G::NEW0, G::NEW4> ce(per_tile(tid));
                const uint8_t* p = (ce.right ? Rf : Lf) + (int64_t)(y0 - R + staged_row(ce.q, 0)) * a.pitch +
                                   ((ce.right ? nxr : nxl) + ce.dx);
                // (rows relative to the group's first: staged_row(q, i) - staged_row(q, 0) does not depend on q)
#pragma unroll
                for (int i = 0; i < 8; ++i) __builtin_memcpy(&pw[i], p + (int64_t)staged_row(0, i) * a.pitch, 4);
            }
        };
        // NP = 1: before the disparity loops, which cover the latency.  NP = 2: after both loops, whose order needs
        // the eight registers; the fold and the epilogue are between the loads and their use
        if constexpr (NP == 1) issue_prefetch();

        __syncthreads();

        // The run's last tile: the grab for the next run goes out now, its latency under the disparity loops, and
        // into the LDS word behind them, ahead of the barrier every wave passes before it reads the word
        uint32_t next_grab = 0;
        const bool draw = queued && tile + 1 == t_end && tid == 0;
        if constexpr (queued) {
            if (draw) next_grab = atomicAdd(queue, 1u);
        }

        // One loop over [lo, hi) in the compiler's order; MASKED: with the c >= d and c < W mask of the staged columns
        // and the d <= W - x mask of the outputs.  The NP = 1 kernels run it for both parts of a wave's range; the
        // NP = 2 kernels do not instantiate it (run_paired below), its NP = 2 arms state the same arithmetic
        auto run = [&](auto masked_c, const int lo, const int hi) {
            constexpr bool MASKED = decltype(masked_c)::value;
            // NP = 2: two disparities per pass; an odd range ends with its last d twice (the same keys: min3 is
            // unchanged, and no column outside the loop's own range is read)
#pragma unroll 1
            for (int d = lo; d < hi; d += NP) {
                const int dd[2] = {d, min(d + 1, hi - 1)};
                int raddr[NP];
                float c2v[NP];
                f4 c2[NP];
#pragma unroll
                for (int p = 0; p < NP; ++p) {
                    raddr[p] = slot(l16 + DMAX + d_lo - dd[p], g);
                    c2v[p] = c2base + (float)dd[p];
                    c2[p] = f4{c2v[p], c2v[p], c2v[p], c2v[p]};
                }
                // L does not depend on d, but holding it would take 32 more registers and a wave per SIMD: the
                // d-dependent zero (d >= 0) keeps the reads inside the loop, once per pair
                const int laddr_d = laddr + (int)((uint32_t)d >> 31);
                // t[p][ob]: the packed D1 of two adjacent column blocks of disparity p, a stage-2 B operand.  Even
                // blocks go to its low half and odd blocks to its high half, so no half is ever copied; bh or bhs
                // matches the order.  With NXB = 4 the last output block (cb == 4) pairs block 3 with the stale block
                // 2: with the left block in the high half the stale columns meet only outputs past TOX, which are
                // never written
                u4 t[NP][NOB];
#pragma unroll
                for (int cb = 0; cb <= NXB; ++cb) {
                    if (cb < 4) {
                        const u4 l0 = *reinterpret_cast<const u4*>(lsm + laddr_d + cb * 16 * kColB);
                        const u4 l1 = *reinterpret_cast<const u4*>(lsm + (laddr_d ^ 64) + cb * 16 * kColB);
#pragma unroll
                        for (int p = 0; p < NP; ++p) {
                            const u4 r0 = *reinterpret_cast<const u4*>(rsm + raddr[p] + cb * 16 * kColB);
                            const u4 r1 = *reinterpret_cast<const u4*>(rsm + (raddr[p] ^ 64) + cb * 16 * kColB);
                            // a lane is one image column for all eight AD registers: its mask rides on their AND
                            uint32_t keep = kAbsBits;
                            // (d <= c < W as one unsigned compare: d <= W in every pass.  The scalar part goes through
                            // readfirstlane so that no per-lane part of it is hoisted and held over the loop)
                            if constexpr (MASKED) {
                                const int c0 = __builtin_amdgcn_readfirstlane(x0 - R + 16 * cb - dd[p]);
                                keep = (uint32_t)(l16 + c0) < (uint32_t)(W - dd[p]) ? kAbsBits : 0u;
                            }
                            const u4 ad0 = abs_diff(l0, r0, keep);
                            const u4 ad1 = abs_diff(l1, r1, keep);
                            // output row blocks 0..NOB-1 of this column block from the two 32-row chunks as they are
                            // read: the middle block from both, 16 rows down in the first and 16 up in the second.  The
                            // three views of run_paired cost this loop, which the compiler orders, its order
                            f4 sv[4];
                            sv[0] = mfma(ad0, bv, c1);
                            sv[1] = mfma(ad0, bv4, c1);
                            sv[1] = mfma(ad1, bvp, sv[1]);
                            sv[2] = mfma(ad1, bv, c1);
                            if constexpr (NOB == 4) sv[3] = mfma(ad1, bv4, c1);
#pragma unroll
                            for (int ob = 0; ob < NOB; ++ob) {
                                const uint2 pk = pack_f16(sv[ob]);
                                t[p][ob][2 * (cb & 1)] = pk.x;
                                t[p][ob][2 * (cb & 1) + 1] = pk.y;
                            }
                        }
                    }
                    // NP = 2: the scheduler takes stage 1 and stage 2 of a column block as regions of their own: over
                    // the whole pass its latency-hiding order needs more than 168 registers and it falls back to source
                    // order (65 s_nop per pass instead of 20)
                    if constexpr (NP == 2) __builtin_amdgcn_sched_barrier(0);
                    if (cb >= 1) {
                        const int xb = cb - 1;
                        // an output column past W - d starts from +inf: the products are finite, so its accumulator
                        // stays +inf (kInfBits exactly) for every row block, and the min and the epilogue read it as
                        // "no valid d".  Built per column block, so it is not held over the pass
                        f4 c2x[NP];
#pragma unroll
                        for (int p = 0; p < NP; ++p) {
                            c2x[p] = c2[p];
                            if constexpr (MASKED) {
                                // element i is output column x0 + 16 xb + 4g + i, valid for d <= W - x.  No scalar skip
                                // of blocks that are valid throughout: a branch inside the pass spills
                                const int e = __builtin_amdgcn_readfirstlane(W - x0 - 16 * xb - dd[p]) - 4 * g;
#pragma unroll
                                for (int i = 0; i < 4; ++i)
                                    c2x[p][i] = i <= e ? c2v[p] : __builtin_bit_cast(float, kInfBits);
                            }
                        }
#pragma unroll
                        for (int ob = 0; ob < NOB; ++ob) {
                            u4 o[NP];
#pragma unroll
                            for (int p = 0; p < NP; ++p)
                                o[p] = __builtin_bit_cast(u4, mfma((cb & 1) ? bh : bhs, t[p][ob], c2x[p]));
#pragma unroll
                            for (int i = 0; i < 4; ++i) {
                                uint32_t k = o[0][i];
#pragma unroll
                                for (int p = 1; p < NP; ++p) k = min(k, o[p][i]);
                                best[ob][xb][i] = min(best[ob][xb][i], k);   // NP = 2: v_min3_u32
                            }
                        }
                    }
                    if constexpr (NP == 2) __builtin_amdgcn_sched_barrier(0);
                }
            }
        };
        // The loops of two disparities per pass, the same arithmetic as run() in an order that gives every
        // MFMA vector work of its own wave that does not wait for it.  A column block is a sequence of
        // slots, one MFMA and two to four vector instructions each, a scheduling barrier after every slot, so the source
        // order is the machine order:
        //   stage 1   a disparity's eight AD registers are one tuple, filled chunk 0 (4 v_pk_add_f16 + 4 v_and_b32), then
        //             chunk 1 by halves, p0 and p1 alternating; row block ob is one MFMA on registers 2 ob .. 2 ob + 3
        //             (ad_view): the first once chunk 0 is there, the middle one after the first half of
        //             chunk 1, the last after the second.  An MFMA issues half a quad or more after the last AND it
        //             reads; a convert follows the sum it reads by four MFMAs
        //   stage 2   of the output block to the left: its six MFMAs in row block order under the last converts and
        //             the mins of the rows done; the mins of the last row block wait for the first AD quad of the next
        //             column block
        //   reads     chunk 0 of the next block goes out before the last two stage-2 MFMAs (one slot earlier the
        //             R = 1, d_max = 64 queue kernel spills a register), chunk 1 with the
        //             block's first quad (the R read its last quad needs one slot later), so only the first block of
        //             a pass begins with a wait (sending that block's reads out from the pass before was measured and
        //             bought nothing).  Reading all six ahead, or holding the next tile's staging loads
        //             over these loops as NP = 1 does, does not fit in 168 registers
        // Both loops of a wave are this one body, [lo, mid) unmasked and [mid, hi) masked: the masked
        // instantiation is the unmasked one plus the mask work, and takes over the carried values where the first
        // loop leaves them (mid - lo is even).
        //   AD mask   keep = kAbsBits or 0 per (column block, p) from d <= c < W as one unsigned compare of
        //             l16 + c0 against W - d, both scalars carried and stepped by -2 per pass; made ahead of the
        //             block's first quad, in the slots of the second and third stage-2 MFMA of the block to the left
        //             (the first block's at the head of the pass, behind its reads)
        //   key mask  element i of output block xb is valid for d <= W - x, i.e. 4 i <= e4 for p = 0 and
        //             4 (i + 1) <= e4 for p = 1 with the one per-lane operand e4 = 4 (W - x0 - 16 xb - d) - 16 g; made
        //             from the carried c2[p] in the two slots before the block's stage 2, under stage-1 MFMAs, which
        //             do not read it (in the last output block, which has no stage 1, ahead of its first two MFMAs)
        // In an odd last pass p = 1 repeats d: its masks are p = 0's (`one` is 0), as its R address is
        auto run_paired = [&](auto np_c, const int lo, const int mid, const int hi) {
            static_assert(decltype(np_c)::value == 2 && NOB == 3, "the paired loop");
            auto slot_end = [] { __builtin_amdgcn_sched_barrier(0); };
            // An empty asm that takes a value and gives it back (no instruction is emitted).  In a slot: a value that
            // only the next pass reads is computed there, not at the loop's end.  At the head of a pass: a value that
            // does not change stays in its registers and what is read through it stays in the loop
            auto pin = [](auto& v) { asm volatile("" : "+v"(v)); };
            // the two keys of a pixel against its best: v_min3_u32
            auto mins = [&](int ob, int x, const u4& o0, const u4& o1) {
#pragma unroll
                for (int i = 0; i < 4; ++i) best[ob][x][i] = min(best[ob][x][i], min(o0[i], o1[i]));
            };
            // Carried from pass to pass, stepped in the last output block's slots instead of rebuilt at the head of a
            // pass, ahead of its first reads:
            //   c2[p]   the key constant of disparity d + p as a splat, + 2.0 per pass.  The odd last pass repeats
            //           d = hi - 1 as p = 1 (dd[1]) and labels it d + 1: the same cost as p = 0's key with a larger low
            //           byte, so it loses every min against p = 0's key and changes nothing
            //   rcol    byte offset of p = 0's column l16 + DMAX + d_lo - d, - 2 columns per pass.  slot()'s swizzle
            //           (col >> 1) & 7 is bits 8..10 of it, so an address is a shift, an and-xor and an add
            //   raddr[] the two R addresses of the pass; p = 1 reads one column to the left, or p = 0's in an odd
            //           last pass (dd[] decides, as it does in run()).  The clamp is against the wave's own hi, at most
            //           the tile's d_end <= d_lo + DMAX, so every staged column read lies in [0, RC)
            // The addresses are LDS addresses, not offsets into smem[] to which every read adds the array's own
            // address again: smem is aligned to a whole swizzle period, so the swizzle of an address is the swizzle
            // of the offset
            const int g16 = g << 4;
            auto swz = [&](int colb) { return colb + (((colb >> 4) & 0x70) ^ g16); };
            auto lds_u4 = [](int addr) { return *(const __attribute__((address_space(3))) u4*)(uint32_t)addr; };
            const int lds0 = (int)(uint32_t)(uintptr_t)(const __attribute__((address_space(3))) uint8_t*)smem;
            auto raddr_at = [&](int colb, int d, int (&ra)[2]) {
                ra[0] = swz(colb);
                ra[1] = swz(colb - (d + 1 < hi ? kColB : 0));
            };
            int rcol = lds0 + G::L_BYTES + (l16 + DMAX + d_lo - lo) * kColB;
            int raddr[2];
            raddr_at(rcol, lo, raddr);
            f4 c2[2];
#pragma unroll
            for (int p = 0; p < 2; ++p) {
                const float c2v = c2base + (float)(lo + p);
                c2[p] = f4{c2v, c2v, c2v, c2v};
            }
            const f4 two = {2.0f, 2.0f, 2.0f, 2.0f};
            // L does not depend on d, and as in run() its reads stay inside the loop, once per pair: here the two
            // chunk addresses pass through an empty asm per pass instead of a d-dependent zero
            int laddr_c[2] = {lds0 + laddr, (lds0 + laddr) ^ 64};
            // stage 1's C operand, held: left to the compiler it is rebuilt from scalar registers in every pass
            f4 c1p = c1;
            // the eight AD registers of each disparity, one tuple for the whole loop: every pass writes all of them
            // before it reads them
            u8 ad8[2] = {};
            // The masks' scalars: wd = W - d, c0s = x0 - R - d, the image column of lane 0's staged column less d.  They
            // pass through an empty asm in every pass, so that nothing per-lane is derived from them ahead of the loop
            // and held over it
            int wd = W - mid, c0s = x0 - R - mid;
            auto pass = [&](auto masked_c, const int d) {
                constexpr bool MASKED = decltype(masked_c)::value;
                pin(laddr_c[0]);
                pin(laddr_c[1]);
                pin(c1p);
                // 1 where p = 1 is d + 1, 0 where it repeats d (the odd last pass)
                const int one = d + 1 < hi ? 1 : 0;
                if constexpr (MASKED) {
                    asm volatile("" : "+s"(wd));
                    asm volatile("" : "+s"(c0s));
                }
                u4 t[2][NOB];
                u4 lq[2], rq[2][2];   // [chunk], [p][chunk] of the block whose reads are out
                // the reads of 32-row chunk c of column block cb
                auto fetch_l = [&](int cb, int c) { lq[c] = lds_u4(laddr_c[c] + cb * 16 * kColB); };
                auto fetch_r = [&](int cb, int p, int c) {
                    rq[p][c] = lds_u4((raddr[p] ^ (64 * c)) + cb * 16 * kColB);
                };
                auto fetch = [&](int cb, int c) {
                    fetch_l(cb, c);
                    fetch_r(cb, 0, c);
                    fetch_r(cb, 1, c);
                };
                uint32_t keep[2] = {kAbsBits, kAbsBits};
                f4 c2x[2];
                auto mk_keep = [&](int cb, int p) {
                    if constexpr (MASKED)
                        keep[p] = (uint32_t)(l16 + (c0s + 16 * cb - p * one)) < (uint32_t)(wd - p * one) ? kAbsBits : 0u;
                };
                auto mk_c2x = [&](int xb, int p) {
                    if constexpr (MASKED) {
                        const int e4 = 4 * (wd - x0 - 16 * xb) - g16;
#pragma unroll
                        for (int i = 0; i < 4; ++i)
                            c2x[p][i] = 4 * (i + p * one) <= e4 ? c2[p][0] : __builtin_bit_cast(float, kInfBits);
                    }
                };
                // the next pass's R addresses, once this pass's last R read is out (the unmasked loop's last pass steps
                // to `mid`, the masked loop's first).  The step is a scalar, 0 in the range's last pass, whose addresses
                // nobody reads: with a literal step the slot compiles to one instruction and six wait states more
                auto step_addr = [&] {
                    rcol -= d + 2 < hi ? 2 * kColB : 0;
                    raddr_at(rcol, d + 2, raddr);
                    pin(raddr[0]);
                    pin(raddr[1]);
                };
                fetch(0, 0);
                mk_keep(0, 0);
                mk_keep(0, 1);
                u4 om[2];   // stage 2 of the last row block, carried to the next column block's first quad
#pragma unroll
                for (int cb = 0; cb <= NXB; ++cb) {
                    const bool s1 = cb < 4, s2 = cb >= 1;
                    const int xb = cb - 1;
                    f4 sv[2][NOB];
                    u4 o[2][NOB];
                    // elements 2h, 2h + 1 of AD quad (p, chunk c): registers 4c + 2h, 4c + 2h + 1 of ad8[p]
                    auto half = [&](int p, int c, int h) {
#pragma unroll
                        for (int m = 2 * h; m < 2 * h + 2; ++m) {
                            const uint32_t lm = lq[c][m], rm = rq[p][c][m];
                            const h2 df = __builtin_bit_cast(h2, lm) - __builtin_bit_cast(h2, rm);
                            ad8[p][4 * c + m] = __builtin_bit_cast(uint32_t, df) & keep[p];
                        }
                    };
                    // row block ob of disparity p: its view of the eight AD registers against the one band
                    auto stage1 = [&](int p, int ob) { sv[p][ob] = mfma(ad_view(ad8[p], ob), bv, c1p); };
                    auto cvt = [&](int p, int ob) {
                        const uint2 pk = pack_f16(sv[p][ob]);
                        t[p][ob][2 * (cb & 1)] = pk.x;
                        t[p][ob][2 * (cb & 1) + 1] = pk.y;
                    };
                    auto stage2 = [&](int ob, int p) {
                        o[p][ob] = __builtin_bit_cast(u4, mfma((cb & 1) ? bh : bhs, t[p][ob], MASKED ? c2x[p] : c2[p]));
                    };
                    if (s1) {
                        fetch_l(cb, 1);
                        fetch_r(cb, 0, 1);
                        half(0, 0, 0);
                        half(0, 0, 1);
                        if (cb >= 2) mins(2, xb - 1, om[0], om[1]);
                        slot_end();
                        fetch_r(cb, 1, 1);
                        stage1(0, 0);
                        half(1, 0, 0);
                        half(1, 0, 1);
                        slot_end();
                        half(0, 1, 0);
                        if (cb == NXB) step_addr();   // NXB = 3: the pass's last R read is out
                        slot_end();
                        stage1(1, 0);
                        half(1, 1, 0);
                        slot_end();
                        stage1(0, 1);
                        half(0, 1, 1);
                        slot_end();
                        stage1(1, 1);
                        half(1, 1, 1);
                        slot_end();
                        stage1(0, 2);
                        cvt(0, 0);
                        if (s2) mk_c2x(xb, 0);
                        slot_end();
                        stage1(1, 2);
                        cvt(1, 0);
                        if (s2) mk_c2x(xb, 1);
                        slot_end();
                        if (s2) stage2(0, 0);
                        cvt(0, 1);
                        slot_end();
                        if (s2) stage2(0, 1);
                        cvt(1, 1);
                        if (cb + 1 < 4) mk_keep(cb + 1, 0);
                        slot_end();
                        if (s2) stage2(1, 0);
                        cvt(0, 2);
                        if (cb + 1 < 4) mk_keep(cb + 1, 1);
                        slot_end();
                        if (s2) stage2(1, 1);
                        cvt(1, 2);
                        slot_end();
                        if (cb + 1 < 4) fetch(cb + 1, 0);
                        if (s2) {
                            stage2(2, 0);
                            mins(0, xb, o[0][0], o[1][0]);
                            slot_end();
                            stage2(2, 1);
                            slot_end();
                            mins(1, xb, o[0][1], o[1][1]);
                            slot_end();
                            om[0] = o[0][2];
                            om[1] = o[1][2];
                        }
                    } else {
                        // the last output block: both halves of t are there; the next pass's addresses go under its
                        // first MFMAs
                        mk_c2x(xb, 0);
                        stage2(0, 0);
                        step_addr();
                        mk_c2x(xb, 1);
                        stage2(0, 1);
                        slot_end();
                        stage2(1, 0);
                        mins(2, xb - 1, om[0], om[1]);
                        slot_end();
                        stage2(1, 1);
                        slot_end();
                        stage2(2, 0);
                        mins(0, xb, o[0][0], o[1][0]);
                        slot_end();
                        stage2(2, 1);
                        slot_end();
                        mins(1, xb, o[0][1], o[1][1]);
                        slot_end();
                        om[0] = o[0][2];
                        om[1] = o[1][2];
                    }
                }
                mins(2, NXB - 1, om[0], om[1]);
                // (after the last MFMA that reads them: a write under it would wait for its C operand)
                c2[0] += two;
                c2[1] += two;
                if constexpr (MASKED) {
                    wd -= 2;
                    c0s -= 2;
                }
                slot_end();
            };
#pragma unroll 1
            for (int d = lo; d < mid; d += 2) pass(std::false_type{}, d);
#pragma unroll 1
            for (int d = mid; d < hi; d += 2) pass(std::true_type{}, d);
        };
        if constexpr (NP == 2) {
            run_paired(std::integral_constant<int, NP>{}, dw_lo, dw_m, dw_hi);
            // (zeros on the other path: an undefined value would be taken as last tile's and held over the loop)
            if (!prefetch) {
#pragma unroll
                for (int i = 0; i < 8; ++i) pw[i] = 0;
            }
            issue_prefetch();
        } else {
            run(std::false_type{}, dw_lo, dw_m);
            run(std::true_type{}, dw_m, dw_hi);
        }
        if constexpr (queued) {
            if (draw) *qword = next_grab;
        }

        __syncthreads();   // every wave is done with the staged tiles: the fold plane aliases them

        // ---- fold the waves (same lane = same pixels in every wave) through one LDS plane ----
        uint32_t* fold = reinterpret_cast<uint32_t*>(smem);   // [TOY][FOLD] f32 bit patterns
        if (wave == 0) {
#pragma unroll
            for (int ob = 0; ob < NOB; ++ob)
#pragma unroll
                for (int xb = 0; xb < NXB; ++xb)
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        fold[(16 * ob + l16) * G::FOLD + 16 * xb + 4 * g + i] = best[ob][xb][i];
        }
        __syncthreads();
        if (wave != 0) {
#pragma unroll
            for (int ob = 0; ob < NOB; ++ob)
#pragma unroll
                for (int xb = 0; xb < NXB; ++xb)
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        atomicMin(&fold[(16 * ob + l16) * G::FOLD + 16 * xb + 4 * g + i], best[ob][xb][i]);
        }
        __syncthreads();
        uint8_t* Df = a.disp ? a.disp + (int64_t)frame * a.out_frame_stride : nullptr;
        uint32_t* Kf = a.keys ? a.keys + (int64_t)frame * W * H : nullptr;
        // lane = output column, rows over the waves
        if (lane < G::TOX && x0 + lane < W) {
            const int ylim = min(G::TOY, H - y0);
            uint8_t* drow = Df ? Df + (int64_t)y0 * a.out_pitch + x0 + lane : nullptr;
            uint32_t* krow = Kf ? Kf + (int64_t)y0 * W + x0 + lane : nullptr;
            for (int j = wave; j < ylim; j += kNW) {
                // the f32 key to its integer (+inf: no valid d), then the seed
                const uint32_t kb = fold[j * G::FOLD + lane];
                const uint32_t kf = kb >= kInfBits ? 0xFFFFFFFFu : (uint32_t)__builtin_bit_cast(float, kb);
                const uint32_t k = min(kf, a.seed_key);
                if (drow) drow[(int64_t)j * a.out_pitch] = k < a.thresh_key ? (uint8_t)(k & 0xFFu) : (uint8_t)0;
                if (krow) krow[(int64_t)j * W] = k;
            }
        }

        // ---- the next tile of the range, or the first of the next run ----
        if (tile + 1 == t_end) {
            if constexpr (!queued) break;
            take_run();
            if (t_begin >= t_end) break;
            tile = t_begin - 1;
            frame = t_begin / tiles;
            ty = (t_begin - frame * tiles) / tiles_x;
            tx = t_begin - frame * tiles - ty * tiles_x;
            carried = false;
        } else {
            carried = carry_next;
            if (++tx == tiles_x) {
                tx = 0;
                if (++ty == tiles_y) {
                    ty = 0;
                    ++frame;
                }
            }
        }
        if (!carried) {
            __syncthreads();   // the fold plane is read: the next tile stages over it
            continue;
        }
        // The right-hand neighbour: its band is this one moved down by TOX columns (best[] is dead: through registers,
        // each side with its own swizzle, since the shift changes (col >> 1) & 7), and TOX new columns.  The kept
        // columns lie past the fold plane.  Threads past the last 16-B unit repeat it: no branch, the same bytes
        const int mt = per_tile(tid);
        u4 mv[G::MOVE_U];
#pragma unroll
        for (int i = 0; i < G::MOVE_U; ++i) {
            const int u = min(mt + i * kThreads, G::KEEP * 8 - 1);
            mv[i] = *reinterpret_cast<const u4*>(rsm + slot((u >> 3) + G::TOX, u & 7));
        }
        __syncthreads();   // the band and the fold plane are read
#pragma unroll
        for (int i = 0; i < G::MOVE_U; ++i) {
            const int u = min(mt + i * kThreads, G::KEEP * 8 - 1);
            *reinterpret_cast<u4*>(rsm + slot(u >> 3, u & 7)) = mv[i];
        }
        const CarriedElem<G::NEW0, G::NEW4> ce(mt);
        if (!prefetch) {   // an edge tile: the guarded loads, now
#pragma unroll
            for (int i = 0; i < 8; ++i)
                pw[i] = ld_image_u32(ce.right ? Rf : Lf, y0 - R + staged_row(ce.q, i), (ce.right ? nxr : nxl) + ce.dx,
                                     W, H, a.pitch);
        }
        stage_pack(pw, ce.right ? rsm : lsm, ce.col, ce.q);
    }
}

template <int R, int DMAX, int NP>
__global__ __launch_bounds__(kThreads, 3) void box_mfma_kernel(MatchArgs a, int tiles_x, int tiles_y, int per,
                                                                int rem) {
    box_mfma_tiles<R, DMAX, NP, true, false>(a, tiles_x, tiles_y, per, rem, nullptr);
}

// The paired loop's workgroups drawing runs of `total` tiles from the counter `queue`
template <int R, int DMAX>
__global__ __launch_bounds__(kThreads, 3) void box_mfma_queue_kernel(MatchArgs a, int tiles_x, int tiles_y, int total,
                                                                      uint32_t* queue) {
    box_mfma_tiles<R, DMAX, 2, true, true>(a, tiles_x, tiles_y, total, 0, queue);
}

// One d per pass, one tile per workgroup (what auto launches at NP = 1): with the tile loop around it the NP = 1
// disparity loop loses the scheduler's order (42 s_nop per pass instead of 4) whatever its register count
template <int R, int DMAX>
__global__ __launch_bounds__(kThreads, 3) void box_mfma_tile_kernel(MatchArgs a, int tiles_x, int tiles_y) {
    box_mfma_tiles<R, DMAX, 1, false, false>(a, tiles_x, tiles_y, 1, 0, nullptr);
}

// Static ranges launched per resident slot in auto mode, where the launch does not draw from the queue (no counter
// from the caller, or box_queue_workgroups says no: few tiles per slot).  One static range per slot is the slowest form
// (1080p D = 128 r = 5 x 128 frames: 5.40 ms against 5.07 for one tile per workgroup): the three waves of a SIMD keep
// their age order for the whole launch, equal shares go to workgroups that do not run at equal speed, and the launch
// ends with the youngest.  Shorter ranges let the dispatcher even that out: 2 / 4 / 8 / 16 per slot 5.14 / 4.94 / 4.98 /
// 4.94 ms, D = 256 x 32 frames 2.48 / 2.42 / 2.39 / 2.39 (profiles/microbench/box_mfma_rows_ab.txt).  The queue is the
// other cure: one workgroup per slot, each taking what it has time for
constexpr int kRangesPerSlot = 16;

// workgroups: 0 auto, n >= 1 that many static ranges, at most one per tile.  Auto: with a counter from the caller,
// box_queue_workgroups(.., queue_workgroups) workgroups that draw their tiles from it, else kRangesPerSlot static
// ranges of tiles per resident workgroup slot
template <int R, int DMAX, int NP>
hipError_t launch_rdp(const MatchArgs& a, int batch, hipStream_t s, int workgroups, uint32_t* queue,
                      int queue_workgroups) {
    using G = MG<R, DMAX, NP>;
    static_assert(NP == box_mfma_np(R, NP == 1 ? 32 : DMAX) && G::TOX == box_mfma_tox(R, NP) &&
                      G::TOY == box_mfma_toy(R, NP),
                  "bm_box_plan.h states this tile");
    const int tiles_x = (a.W + G::TOX - 1) / G::TOX;
    const int tiles_y = (a.H + G::TOY - 1) / G::TOY;
    const int64_t total = (int64_t)tiles_x * tiles_y * batch;
    if (total <= 0 || total > 0x7FFFFFFF || workgroups < 0) return hipErrorInvalidValue;
    int64_t n = workgroups;
    // one d per pass (short ranges at r <= 2): a tile's loop is too short to pay for the move and its barrier, auto
    // keeps one tile per workgroup (1080p D = 32 r = 2 x 32 frames: 0.405 ms against 0.509 with ranges)
    if constexpr (NP == 1) {
        if (n == 0 || n >= total) {
            hipLaunchKernelGGL((box_mfma_tile_kernel<R, DMAX>), dim3((unsigned)total), dim3(kThreads),
                               (size_t)G::LDS_BYTES, s, a, tiles_x, tiles_y);
            return hipGetLastError();
        }
    }
    if constexpr (NP == 2) {
        if (n == 0 && queue) {
            int slots = 0;
            hipError_t e = resident_workgroups(reinterpret_cast<const void*>(&box_mfma_queue_kernel<R, DMAX>), kThreads,
                                               (size_t)G::LDS_BYTES + kQueueLdsBytes, &slots);
            if (e != hipSuccess) return e;
            const int q = box_queue_workgroups(NP, a.d_hi - a.d_lo, total, slots, workgroups, queue_workgroups);
            if (q > 0) {
                // the counter is zeroed on the launch's stream, so launches of one handle follow each other on it
                e = hipMemsetAsync(queue, 0, sizeof(uint32_t), s);
                if (e != hipSuccess) return e;
                hipLaunchKernelGGL((box_mfma_queue_kernel<R, DMAX>), dim3((unsigned)q), dim3(kThreads),
                                   (size_t)G::LDS_BYTES + kQueueLdsBytes, s, a, tiles_x, tiles_y, (int)total, queue);
                return hipGetLastError();
            }
        }
    }
    if (n == 0) {
        int slots = 0;
        hipError_t e = resident_workgroups(reinterpret_cast<const void*>(&box_mfma_kernel<R, DMAX, NP>), kThreads,
                                           (size_t)G::LDS_BYTES, &slots);
        if (e != hipSuccess) return e;
        n = (int64_t)slots * kRangesPerSlot;
    }
    if (n > total) n = total;
    hipLaunchKernelGGL((box_mfma_kernel<R, DMAX, NP>), dim3((unsigned)n), dim3(kThreads), (size_t)G::LDS_BYTES, s, a,
                       tiles_x, tiles_y, (int)(total / n), (int)(total % n));
    return hipGetLastError();
}

template <int R, int DMAX>
hipError_t launch_rd(const MatchArgs& a, int batch, hipStream_t s, int workgroups, uint32_t* queue,
                     int queue_workgroups) {
    // short ranges at r <= 2 keep one d per pass on 62- / 60-row tiles: 1080p x 32 frames, D = 8 r = 1 0.206 against
    // 0.221 ms, D = 32 r = 2 0.396 against 0.404; from r = 3 or D = 48 on the paired loop is level or ahead
    // (profiles/microbench/box_mfma_pairs_ab.txt)
    if constexpr (DMAX == 64 && R <= 2) {
        if (a.d_hi - a.d_lo <= 32) return launch_rdp<R, DMAX, 1>(a, batch, s, workgroups, queue, queue_workgroups);
    }
    return launch_rdp<R, DMAX, 2>(a, batch, s, workgroups, queue, queue_workgroups);
}

template <int R>
hipError_t launch_r(const MatchArgs& a, int batch, hipStream_t s, int workgroups, uint32_t* queue,
                    int queue_workgroups) {
    const int dspan = a.d_hi - a.d_lo;
    if (dspan <= 64) return launch_rd<R, 64>(a, batch, s, workgroups, queue, queue_workgroups);
    if (dspan <= 128) return launch_rd<R, 128>(a, batch, s, workgroups, queue, queue_workgroups);
    if (dspan <= 192) return launch_rd<R, 192>(a, batch, s, workgroups, queue, queue_workgroups);
    return launch_rd<R, 256>(a, batch, s, workgroups, queue, queue_workgroups);
}

}  // namespace

hipError_t launch_box_match_mfma(const MatchArgs& a, int batch, hipStream_t s, int workgroups, uint32_t* queue,
                                 int queue_workgroups) {
    if (!box_mfma_scope(box_geom(a, batch), a.valid_mode)) return hipErrorInvalidValue;
    return with_radius<1, kMaxFastRadius>(a.radius, hipErrorInvalidValue, [&](auto r) {
        return launch_r<decltype(r)::value>(a, batch, s, workgroups, queue, queue_workgroups);
    });
}

}  // namespace sm
