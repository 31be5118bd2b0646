// mosrx_steer.hip — queue steering: a stable partition of a batch's frame
// indices by the queue byte of the records the classify kernels wrote
// (GetRSSCPUCore, core/src/util.c:114-131), the sort a NIC's RSS does into
// per-core rx queues.
//
// Three ordinary launches on one stream, over tiles of MOSRX_STEER_TILE frames:
//   1. histogram  tile_hist[tile][256]: each workgroup counts its tile's keys
//   2. scan       per batch: exclusive prefix over the batch's tiles for each
//                 of the 256 columns (each tile's base per queue overwrites
//                 its histogram row), exclusive prefix over queues -> qstart
//   3. scatter    each workgroup re-reads its tile and stores
//                 idx[qstart[q] + base[tile][q] + rank] = i
// No workgroup waits on another within a launch; every loop's bound is known
// at its entry; every idx store is guarded by pos < n of its batch.
//
// A frame's rank among the frames of its key is positional: its 64-frame
// slice's rows come in index order (a prefix over per-slice counts in LDS,
// never the order waves arrive in), and within a slice it is
// popcount(same_key_mask & lanes_below) (v_mbcnt).  same_key_mask comes from
// one ballot per key bit (8 rounds whatever the keys are; peeling distinct
// keys one ballot each would take up to 64 rounds on a slice of many queues).
//
// With gather outputs (mosrx_gdesc) the scatter launch is its gather form
// (3g below): the same positions, with the frame's record, offset and length
// stored beside idx[pos].  Launches without them run the plain pass unchanged.
//
// With mosrx_sparams.fused the three launches are one kernel, one workgroup per
// batch (mosrx_steer_one_kernel below): for batches of a tile or so, where the
// launches' latency is the cost.  The five kernels above it are untouched by it.
//
// The key of frame i is byte rec_bytes - 3 of its record (mosrx_result.queue,
// mosrx_result8.queue); it is read as the aligned dword that holds it, so a
// wave's key loads are dword loads at a stride of 8 or 16 bytes: the same
// cache lines as the records themselves, each touched once per pass.
#include <hip/hip_runtime.h>
#include <errno.h>
#include <stdint.h>

#include "mosrx_steer.h"

#define STEER_WAVES  (MOSRX_STEER_THREADS / 64u)               // 8
#define STEER_ROWS   (MOSRX_STEER_TILE / 64u)                  // 32 slices of 64 frames per tile
#define STEER_SLICES (STEER_ROWS / STEER_WAVES)                // 4 per wave, consecutive
#define SCAN_THREADS 1024u
#define SCAN_SEGS    (SCAN_THREADS / MOSRX_STEER_BINS)         // 4 groups of 256 column lanes

static_assert(MOSRX_STEER_TILE % 64u == 0 && STEER_ROWS % STEER_WAVES == 0, "tile = whole waves of 64");
static_assert(MOSRX_STEER_BINS == 256u && MOSRX_STEER_QSLOTS == MOSRX_STEER_BINS + 1u, "the key is a byte");

// The batch of workgroup `blk`: the one in the arguments, or by binary search
// of tile_base[] as the batch queue does (find k: tile_base[k] <= blk <
// tile_base[k+1]; empty batches share their successor's base and are skipped).
__device__ __forceinline__ mosrx_sdesc steer_batch(const mosrx_sparams &sp, uint32_t blk)
{
	if (!sp.desc)
		return sp.one;
	uint32_t lo = 0, hi = sp.nb;
	for (int it = 0; it < 32 && hi - lo > 1; it++) {
		const uint32_t mid = (lo + hi) >> 1;
		if (sp.desc[mid].tile_base <= blk)
			lo = mid;
		else
			hi = mid;
	}
	return sp.desc[lo];
}

__device__ __forceinline__ uint32_t steer_key(const uint8_t *rec, uint32_t i, uint32_t rec_bytes)
{
	const uint32_t *p = reinterpret_cast<const uint32_t *>(rec + (uint64_t)i * rec_bytes + (rec_bytes - 4u));
	return (*p >> 8) & 0xFFu;   // byte rec_bytes - 3
}

// The lanes of the wave that hold a valid frame with this lane's key.
__device__ __forceinline__ uint64_t same_key_mask(uint32_t key, bool valid)
{
	uint64_t m = __ballot(valid);
#pragma unroll
	for (int b = 0; b < 8; b++) {
		const bool bit = (key >> b) & 1u;
		const uint64_t set = __ballot(bit);
		m &= bit ? set : ~set;
	}
	return m;
}

__device__ __forceinline__ uint32_t lanes_below(uint64_t m)
{
	return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

// ---- 1. histogram ----------------------------------------------------------
// One LDS atomic per distinct key per 64-frame slice (its first lane adds the
// slice's count), as the classify kernels' reason counters do.
__global__ __launch_bounds__(MOSRX_STEER_THREADS) void mosrx_steer_hist_kernel(mosrx_sparams sp)
{
	__shared__ uint32_t s_bin[MOSRX_STEER_BINS];
	const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
	if (blockIdx.x >= sp.total_tiles)
		return;
	if (t < MOSRX_STEER_BINS)
		s_bin[t] = 0;
	__syncthreads();
	const mosrx_sdesc d = steer_batch(sp, blockIdx.x);
	const uint32_t first = (blockIdx.x - d.tile_base) * MOSRX_STEER_TILE + wave * (STEER_SLICES * 64u);
#pragma unroll
	for (uint32_t s = 0; s < STEER_SLICES; s++) {
		const uint32_t i = first + s * 64u + lane;
		const bool valid = i < d.n;
		const uint32_t key = valid ? steer_key(d.rec, i, sp.rec_bytes) : 0u;
		const uint64_t same = same_key_mask(key, valid);
		if (valid && lanes_below(same) == 0)
			atomicAdd(&s_bin[key], (uint32_t)__builtin_popcountll(same));
	}
	__syncthreads();
	if (t < MOSRX_STEER_BINS)
		sp.hist[(uint64_t)blockIdx.x * MOSRX_STEER_BINS + t] = s_bin[t];
}

// ---- 2. scan ---------------------------------------------------------------
// One workgroup per batch, 4 x 256 lanes: lane (g, col) owns column col of the
// g-th quarter of the batch's tiles, so a huge batch's column walk is spread
// over 1024 lanes and every row access is a coalesced 1 KiB.
__global__ __launch_bounds__(SCAN_THREADS) void mosrx_steer_scan_kernel(mosrx_sparams sp)
{
	__shared__ uint32_t s_seg[SCAN_SEGS][MOSRX_STEER_BINS];
	__shared__ uint32_t s_q[MOSRX_STEER_BINS];
	const uint32_t t = threadIdx.x, col = t & (MOSRX_STEER_BINS - 1u), g = t / MOSRX_STEER_BINS;
	if (blockIdx.x >= (sp.desc ? sp.nb : 1u))
		return;
	const mosrx_sdesc d = sp.desc ? sp.desc[blockIdx.x] : sp.one;
	const uint32_t tiles = (d.n + MOSRX_STEER_TILE - 1u) / MOSRX_STEER_TILE;
	const uint32_t per = (tiles + SCAN_SEGS - 1u) / SCAN_SEGS;
	const uint32_t t0 = min(g * per, tiles), t1 = min(t0 + per, tiles);
	uint32_t *h = sp.hist + (uint64_t)d.tile_base * MOSRX_STEER_BINS + col;
	uint32_t sum = 0;
#pragma unroll 4
	for (uint32_t r = t0; r < t1; r++)
		sum += h[(uint64_t)r * MOSRX_STEER_BINS];
	s_seg[g][col] = sum;
	__syncthreads();
	uint32_t total = 0, before = 0;   // the column's count in the batch, and in the segments before g
#pragma unroll
	for (uint32_t k = 0; k < SCAN_SEGS; k++) {
		const uint32_t v = s_seg[k][col];
		total += v;
		before += k < g ? v : 0u;
	}
	// inclusive prefix over the 256 queues (Hillis-Steele, 8 steps)
	if (g == 0)
		s_q[col] = total;
	__syncthreads();
#pragma unroll
	for (uint32_t o = 1; o < MOSRX_STEER_BINS; o <<= 1) {
		const uint32_t v = (g == 0 && col >= o) ? s_q[col - o] : 0u;
		__syncthreads();
		if (g == 0)
			s_q[col] += v;
		__syncthreads();
	}
	if (g == 0 && d.qstart) {
		d.qstart[col] = s_q[col] - total;
		if (col == MOSRX_STEER_BINS - 1u)
			d.qstart[MOSRX_STEER_BINS] = s_q[col];   // == n: every frame has one key
	}
	// each tile's base per queue: the column's frames in the batch's tiles before it
	uint32_t run = before;
#pragma unroll 4
	for (uint32_t r = t0; r < t1; r++) {
		const uint32_t v = h[(uint64_t)r * MOSRX_STEER_BINS];
		h[(uint64_t)r * MOSRX_STEER_BINS] = run;
		run += v;
	}
}

// ---- 3. scatter ------------------------------------------------------------
__global__ __launch_bounds__(MOSRX_STEER_THREADS) void mosrx_steer_scatter_kernel(mosrx_sparams sp)
{
	// s_row[r][q]: frames of queue q in the tile's r-th slice, then the slice's
	// first position for q in idx[] (rows are slices in index order)
	__shared__ uint32_t s_row[STEER_ROWS][MOSRX_STEER_BINS];
	const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
	if (blockIdx.x >= sp.total_tiles)
		return;
	for (uint32_t j = t; j < STEER_ROWS * MOSRX_STEER_BINS; j += MOSRX_STEER_THREADS)
		(&s_row[0][0])[j] = 0;
	__syncthreads();
	const mosrx_sdesc d = steer_batch(sp, blockIdx.x);
	const uint32_t row0 = wave * STEER_SLICES;
	const uint32_t first = (blockIdx.x - d.tile_base) * MOSRX_STEER_TILE + row0 * 64u;
	uint32_t key[STEER_SLICES], rank[STEER_SLICES];
#pragma unroll
	for (uint32_t s = 0; s < STEER_SLICES; s++) {
		const uint32_t i = first + s * 64u + lane;
		const bool valid = i < d.n;
		key[s] = valid ? steer_key(d.rec, i, sp.rec_bytes) : 0u;
		const uint64_t same = same_key_mask(key[s], valid);
		rank[s] = lanes_below(same);
		if (valid && rank[s] == 0)
			s_row[row0 + s][key[s]] = (uint32_t)__builtin_popcountll(same);   // one writer per (row, key)
	}
	__syncthreads();
	if (t < MOSRX_STEER_BINS) {
		uint32_t run = d.qstart[t] + sp.hist[(uint64_t)blockIdx.x * MOSRX_STEER_BINS + t];
#pragma unroll 8
		for (uint32_t r = 0; r < STEER_ROWS; r++) {
			const uint32_t v = s_row[r][t];
			s_row[r][t] = run;
			run += v;
		}
	}
	__syncthreads();
#pragma unroll
	for (uint32_t s = 0; s < STEER_SLICES; s++) {
		const uint32_t i = first + s * 64u + lane;
		if (i < d.n) {
			const uint32_t pos = s_row[row0 + s][key[s]] + rank[s];
			if (pos < d.n)   // holds by construction; keeps a batch whose records change under the launches in bounds
				d.idx[pos] = i;
		}
	}
}

// ---- 3g. scatter + queue-major gather ---------------------------------------
// The scatter pass with the frame's record, offset and length stored at pos
// next to idx[pos] (mosrx_gdesc).  A lane loads its whole record (one dwordx2
// or dwordx4: the cache lines the key dword alone touches) and takes the key
// from it; lanes of one key in a slice get consecutive positions, so each
// array's stores come in runs.  Same structure as the plain pass: no workgroup
// waits on another, fixed loop bounds, every store under pos < n.
template <uint32_t RB> struct steer_rec;
template <> struct steer_rec<8u> {
	uint2 v;
	__device__ __forceinline__ uint32_t key() const { return (v.y >> 8) & 0xFFu; }
};
template <> struct steer_rec<16u> {
	uint4 v;
	__device__ __forceinline__ uint32_t key() const { return (v.w >> 8) & 0xFFu; }
};

// steer_batch, and the batch's index in the tables
__device__ __forceinline__ uint32_t steer_batch_index(const mosrx_sparams &sp, uint32_t blk)
{
	uint32_t lo = 0, hi = sp.nb;
	for (int it = 0; it < 32 && hi - lo > 1; it++) {
		const uint32_t mid = (lo + hi) >> 1;
		if (sp.desc[mid].tile_base <= blk)
			lo = mid;
		else
			hi = mid;
	}
	return lo;
}

// Its side form (SIDE, mosrx_xdesc) also stores the frame's flow hash, match
// mask and tcpinfo at pos, each array on its own (present or not is uniform
// over the workgroup).  Their loads go out with the record's, before the first
// barrier: they need the frame's index, not its position.  The 12-byte tcpinfo
// moves as three dwords.  SIDE is a template parameter of the body: the plain
// gather kernels are the code they were.
static_assert(sizeof(mosrx_tcpinfo) == 12 && sizeof(mosrx_xdesc) == 48, "side arrays: 12-byte tcpinfo, 48-byte descriptor");

template <uint32_t RB, bool SIDE>
__device__ __forceinline__ void steer_gather_body(const mosrx_sparams &sp)
{
	typedef decltype(steer_rec<RB>::v) vec_t;
	__shared__ uint32_t s_row[STEER_ROWS][MOSRX_STEER_BINS];
	const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
	if (blockIdx.x >= sp.total_tiles)
		return;
	for (uint32_t j = t; j < STEER_ROWS * MOSRX_STEER_BINS; j += MOSRX_STEER_THREADS)
		(&s_row[0][0])[j] = 0;
	__syncthreads();
	mosrx_sdesc d;
	mosrx_gdesc g;
	mosrx_xdesc x = {};
	if (sp.desc) {
		const uint32_t k = steer_batch_index(sp, blockIdx.x);
		d = sp.desc[k];
		g = sp.gdesc[k];
		if constexpr (SIDE)
			x = sp.xdesc[k];
	} else {
		d = sp.one;
		g = sp.gone;
		if constexpr (SIDE)
			x = sp.xone;
	}
	const bool descs = g.qoff != nullptr;   // uniform over the workgroup
	const bool has_fh = SIDE && x.qfhash != nullptr, has_mt = SIDE && x.qmatch != nullptr;
	const bool has_ti = SIDE && x.qtcpinfo != nullptr;
	const uint32_t row0 = wave * STEER_SLICES;
	const uint32_t first = (blockIdx.x - d.tile_base) * MOSRX_STEER_TILE + row0 * 64u;
	steer_rec<RB> r[STEER_SLICES];
	uint32_t key[STEER_SLICES], rank[STEER_SLICES], foff[STEER_SLICES], flen[STEER_SLICES];
	uint32_t ffh[SIDE ? STEER_SLICES : 1u], fmt[SIDE ? STEER_SLICES : 1u];
	uint32_t ti0[SIDE ? STEER_SLICES : 1u], ti1[SIDE ? STEER_SLICES : 1u], ti2[SIDE ? STEER_SLICES : 1u];
#pragma unroll
	for (uint32_t s = 0; s < STEER_SLICES; s++) {
		const uint32_t i = first + s * 64u + lane;
		const bool valid = i < d.n;
		r[s].v = vec_t{};
		foff[s] = flen[s] = 0;
		if constexpr (SIDE) {
			ffh[s] = fmt[s] = 0;
			ti0[s] = ti1[s] = ti2[s] = 0;
		}
		if (valid) {
			r[s].v = *reinterpret_cast<const vec_t *>(d.rec + (uint64_t)i * RB);
			if (descs) {
				foff[s] = g.off[i];
				flen[s] = g.len[i];
			}
			if constexpr (SIDE) {
				if (has_fh)
					ffh[s] = x.fhash[i];
				if (has_mt)
					fmt[s] = x.match[i];
				if (has_ti) {
					const uint32_t *w = reinterpret_cast<const uint32_t *>(x.tcpinfo) + (uint64_t)i * 3u;
					ti0[s] = w[0];
					ti1[s] = w[1];
					ti2[s] = w[2];
				}
			}
		}
		key[s] = valid ? r[s].key() : 0u;
		const uint64_t same = same_key_mask(key[s], valid);
		rank[s] = lanes_below(same);
		if (valid && rank[s] == 0)
			s_row[row0 + s][key[s]] = (uint32_t)__builtin_popcountll(same);   // one writer per (row, key)
	}
	__syncthreads();
	if (t < MOSRX_STEER_BINS) {
		uint32_t run = d.qstart[t] + sp.hist[(uint64_t)blockIdx.x * MOSRX_STEER_BINS + t];
#pragma unroll 8
		for (uint32_t q = 0; q < STEER_ROWS; q++) {
			const uint32_t v = s_row[q][t];
			s_row[q][t] = run;
			run += v;
		}
	}
	__syncthreads();
#pragma unroll
	for (uint32_t s = 0; s < STEER_SLICES; s++) {
		const uint32_t i = first + s * 64u + lane;
		if (i < d.n) {
			const uint32_t pos = s_row[row0 + s][key[s]] + rank[s];
			if (pos < d.n) {   // as the plain pass: every store of the frame under the one guard
				d.idx[pos] = i;
				*reinterpret_cast<vec_t *>(g.qrec + (uint64_t)pos * RB) = r[s].v;
				if (descs) {
					g.qoff[pos] = foff[s];
					g.qlen[pos] = (uint16_t)flen[s];
				}
				if constexpr (SIDE) {
					if (has_fh)
						x.qfhash[pos] = ffh[s];
					if (has_mt)
						x.qmatch[pos] = fmt[s];
					if (has_ti) {
						uint32_t *w = reinterpret_cast<uint32_t *>(x.qtcpinfo) + (uint64_t)pos * 3u;
						w[0] = ti0[s];
						w[1] = ti1[s];
						w[2] = ti2[s];
					}
				}
			}
		}
	}
}

template <uint32_t RB>
__global__ __launch_bounds__(MOSRX_STEER_THREADS) void mosrx_steer_gather_kernel(mosrx_sparams sp)
{
	steer_gather_body<RB, false>(sp);
}

template <uint32_t RB>
__global__ __launch_bounds__(MOSRX_STEER_THREADS) void mosrx_steer_gather_side_kernel(mosrx_sparams sp)
{
	steer_gather_body<RB, true>(sp);
}

// ---- one launch: histogram, scan and scatter / gather in one workgroup --------
// For batches small enough that launch latency, not the walk, is the cost
// (mosrx_sparams.fused): workgroup blockIdx.x takes batch blockIdx.x whole, so
// no workgroup needs another's counts, tile_base and hist are not used, and the
// three phases are separated by __syncthreads() instead of launch boundaries.
//   count  256 LDS bins over the batch's tiles, one atomic per distinct key per slice
//   scan   the 8-step prefix over the bins -> qstart, and each queue's running position
//   place  tile by tile in index order, the scatter / gather body's rows with the
//          queue's running position as their base, then the position moves on by
//          the tile's totals
// A batch of one tile runs count and place from one load: its records (and
// descriptors and side values) stay in registers across the scan, and the bins
// are the column sums of s_row.  n, and with it every loop bound, comes from
// the descriptor at entry and is uniform over the workgroup; every store is
// under pos < n.  FORM: 0 idx only, 1 the gather outputs, 2 gather + side.
#define STEER_ONE_PLAIN  0
#define STEER_ONE_GATHER 1
#define STEER_ONE_SIDE   2
static_assert(MOSRX_STEER_ONE_MAX % MOSRX_STEER_TILE == 0 && MOSRX_STEER_ONE_MAX / MOSRX_STEER_TILE == 32u,
              "the fused form's cap: 32 tiles");

// One tile's frames in a lane's registers: STEER_SLICES frames, what the form gathers of each.
template <uint32_t RB, int FORM> struct steer_one_tile {
	typedef decltype(steer_rec<RB>::v) vec_t;
	static constexpr uint32_t NG = FORM >= STEER_ONE_GATHER ? STEER_SLICES : 1u;
	static constexpr uint32_t NS = FORM == STEER_ONE_SIDE ? STEER_SLICES : 1u;
	uint32_t key[STEER_SLICES], rank[STEER_SLICES];
	steer_rec<RB> r[NG];
	uint32_t foff[NG], flen[NG];
	uint32_t ffh[NS], fmt[NS], ti0[NS], ti1[NS], ti2[NS];
};

// Load tile `tl` of the batch (frames from `first`, this wave's slices) and leave
// the slices' counts per key in s_row (zeroed by the caller, behind a barrier).
template <uint32_t RB, int FORM>
__device__ __forceinline__ void steer_one_load(steer_one_tile<RB, FORM> &f, const mosrx_sdesc &d, const mosrx_gdesc &g,
                                               const mosrx_xdesc &x, uint32_t first, uint32_t row0, uint32_t lane,
                                               uint32_t (*s_row)[MOSRX_STEER_BINS], bool descs, bool has_fh, bool has_mt,
                                               bool has_ti)
{
	typedef typename steer_one_tile<RB, FORM>::vec_t vec_t;
#pragma unroll
	for (uint32_t s = 0; s < STEER_SLICES; s++) {
		const uint32_t i = first + s * 64u + lane;
		const bool valid = i < d.n;
		if constexpr (FORM == STEER_ONE_PLAIN) {
			f.key[s] = valid ? steer_key(d.rec, i, RB) : 0u;
		} else {
			f.r[s].v = vec_t{};
			f.foff[s] = f.flen[s] = 0;
			if constexpr (FORM == STEER_ONE_SIDE) {
				f.ffh[s] = f.fmt[s] = 0;
				f.ti0[s] = f.ti1[s] = f.ti2[s] = 0;
			}
			if (valid) {
				f.r[s].v = *reinterpret_cast<const vec_t *>(d.rec + (uint64_t)i * RB);
				if (descs) {
					f.foff[s] = g.off[i];
					f.flen[s] = g.len[i];
				}
				if constexpr (FORM == STEER_ONE_SIDE) {
					if (has_fh)
						f.ffh[s] = x.fhash[i];
					if (has_mt)
						f.fmt[s] = x.match[i];
					if (has_ti) {
						const uint32_t *w = reinterpret_cast<const uint32_t *>(x.tcpinfo) + (uint64_t)i * 3u;
						f.ti0[s] = w[0];
						f.ti1[s] = w[1];
						f.ti2[s] = w[2];
					}
				}
			}
			f.key[s] = valid ? f.r[s].key() : 0u;
		}
		const uint64_t same = same_key_mask(f.key[s], valid);
		f.rank[s] = lanes_below(same);
		if (valid && f.rank[s] == 0)
			s_row[row0 + s][f.key[s]] = (uint32_t)__builtin_popcountll(same);   // one writer per (row, key)
	}
}

// Store the tile's frames at their positions (s_row: each slice's first position per key).
template <uint32_t RB, int FORM>
__device__ __forceinline__ void steer_one_store(const steer_one_tile<RB, FORM> &f, const mosrx_sdesc &d,
                                                const mosrx_gdesc &g, const mosrx_xdesc &x, uint32_t first, uint32_t row0,
                                                uint32_t lane, const uint32_t (*s_row)[MOSRX_STEER_BINS], bool descs,
                                                bool has_fh, bool has_mt, bool has_ti)
{
	typedef typename steer_one_tile<RB, FORM>::vec_t vec_t;
#pragma unroll
	for (uint32_t s = 0; s < STEER_SLICES; s++) {
		const uint32_t i = first + s * 64u + lane;
		if (i < d.n) {
			const uint32_t pos = s_row[row0 + s][f.key[s]] + f.rank[s];
			if (pos < d.n) {   // as the three-launch passes: every store of the frame under the one guard
				d.idx[pos] = i;
				if constexpr (FORM >= STEER_ONE_GATHER) {
					*reinterpret_cast<vec_t *>(g.qrec + (uint64_t)pos * RB) = f.r[s].v;
					if (descs) {
						g.qoff[pos] = f.foff[s];
						g.qlen[pos] = (uint16_t)f.flen[s];
					}
				}
				if constexpr (FORM == STEER_ONE_SIDE) {
					if (has_fh)
						x.qfhash[pos] = f.ffh[s];
					if (has_mt)
						x.qmatch[pos] = f.fmt[s];
					if (has_ti) {
						uint32_t *w = reinterpret_cast<uint32_t *>(x.qtcpinfo) + (uint64_t)pos * 3u;
						w[0] = f.ti0[s];
						w[1] = f.ti1[s];
						w[2] = f.ti2[s];
					}
				}
			}
		}
	}
}

// Lanes 0..255 hold their queue's count: write qstart (when given) and leave the
// queue's first position in s_run[].  Every lane of the workgroup calls it (barriers).
__device__ __forceinline__ void steer_one_scan(uint32_t t, uint32_t total, uint32_t *s_q, uint32_t *s_run,
                                               uint32_t *qstart)
{
	const bool col = t < MOSRX_STEER_BINS;
	if (col)
		s_q[t] = total;
	__syncthreads();
	// inclusive prefix over the 256 queues (Hillis-Steele, 8 steps)
#pragma unroll
	for (uint32_t o = 1; o < MOSRX_STEER_BINS; o <<= 1) {
		const uint32_t v = (col && t >= o) ? s_q[t - o] : 0u;
		__syncthreads();
		if (col)
			s_q[t] += v;
		__syncthreads();
	}
	if (col) {
		const uint32_t incl = s_q[t];
		s_run[t] = incl - total;
		if (qstart) {
			qstart[t] = incl - total;
			if (t == MOSRX_STEER_BINS - 1u)
				qstart[MOSRX_STEER_BINS] = incl;   // == n: every frame has one key
		}
	}
}

template <uint32_t RB, int FORM>
__global__ __launch_bounds__(MOSRX_STEER_THREADS) void mosrx_steer_one_kernel(mosrx_sparams sp)
{
	// s_row as in the scatter pass; s_run[q]: the next position of queue q (the
	// count phase's bins before the scan); s_q: the scan's working row
	__shared__ uint32_t s_row[STEER_ROWS][MOSRX_STEER_BINS];
	__shared__ uint32_t s_run[MOSRX_STEER_BINS];
	__shared__ uint32_t s_q[MOSRX_STEER_BINS];
	const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
	if (blockIdx.x >= (sp.desc ? sp.nb : 1u))
		return;
	mosrx_sdesc d;
	mosrx_gdesc g = {};
	mosrx_xdesc x = {};
	if (sp.desc) {
		d = sp.desc[blockIdx.x];
		if constexpr (FORM >= STEER_ONE_GATHER)
			g = sp.gdesc[blockIdx.x];
		if constexpr (FORM == STEER_ONE_SIDE)
			x = sp.xdesc[blockIdx.x];
	} else {
		d = sp.one;
		if constexpr (FORM >= STEER_ONE_GATHER)
			g = sp.gone;
		if constexpr (FORM == STEER_ONE_SIDE)
			x = sp.xone;
	}
	// all uniform over the workgroup: one descriptor per workgroup
	const bool descs = FORM >= STEER_ONE_GATHER && g.qoff != nullptr;
	const bool has_fh = FORM == STEER_ONE_SIDE && x.qfhash != nullptr, has_mt = FORM == STEER_ONE_SIDE && x.qmatch != nullptr;
	const bool has_ti = FORM == STEER_ONE_SIDE && x.qtcpinfo != nullptr;
	const uint32_t tiles = (d.n + MOSRX_STEER_TILE - 1u) / MOSRX_STEER_TILE;
	const uint32_t row0 = wave * STEER_SLICES;
	if (tiles == 0) {   // as the scan launch: an empty batch's qstart is 257 zeros, a NULL one is written nowhere
		if (d.qstart && t < MOSRX_STEER_QSLOTS)
			d.qstart[t] = 0;
		return;
	}
	steer_one_tile<RB, FORM> f;
	for (uint32_t j = t; j < STEER_ROWS * MOSRX_STEER_BINS; j += MOSRX_STEER_THREADS)
		(&s_row[0][0])[j] = 0;
	if (t < MOSRX_STEER_BINS)
		s_run[t] = 0;
	__syncthreads();
	if (tiles == 1) {
		// one tile: loaded once; the bins are s_row's column sums
		steer_one_load<RB, FORM>(f, d, g, x, row0 * 64u, row0, lane, s_row, descs, has_fh, has_mt, has_ti);
		__syncthreads();
		uint32_t total = 0;
		if (t < MOSRX_STEER_BINS) {
#pragma unroll 8
			for (uint32_t q = 0; q < STEER_ROWS; q++)
				total += s_row[q][t];
		}
		steer_one_scan(t, total, s_q, s_run, d.qstart);
		if (t < MOSRX_STEER_BINS) {   // (lane t wrote s_run[t] itself)
			uint32_t run = s_run[t];
#pragma unroll 8
			for (uint32_t q = 0; q < STEER_ROWS; q++) {
				const uint32_t v = s_row[q][t];
				s_row[q][t] = run;
				run += v;
			}
		}
		__syncthreads();
		steer_one_store<RB, FORM>(f, d, g, x, row0 * 64u, row0, lane, s_row, descs, has_fh, has_mt, has_ti);
		return;
	}
	// count: the key dword of every frame, tile by tile
	for (uint32_t tl = 0; tl < tiles; tl++) {
		const uint32_t first = tl * MOSRX_STEER_TILE + row0 * 64u;
#pragma unroll
		for (uint32_t s = 0; s < STEER_SLICES; s++) {
			const uint32_t i = first + s * 64u + lane;
			const bool valid = i < d.n;
			const uint32_t key = valid ? steer_key(d.rec, i, RB) : 0u;
			const uint64_t same = same_key_mask(key, valid);
			if (valid && lanes_below(same) == 0)
				atomicAdd(&s_run[key], (uint32_t)__builtin_popcountll(same));
		}
	}
	__syncthreads();
	steer_one_scan(t, t < MOSRX_STEER_BINS ? s_run[t] : 0u, s_q, s_run, d.qstart);
	// place: s_row is zero on entry to every round
	for (uint32_t tl = 0; tl < tiles; tl++) {
		const uint32_t first = tl * MOSRX_STEER_TILE + row0 * 64u;
		steer_one_load<RB, FORM>(f, d, g, x, first, row0, lane, s_row, descs, has_fh, has_mt, has_ti);
		__syncthreads();
		if (t < MOSRX_STEER_BINS) {
			uint32_t run = s_run[t];
#pragma unroll 8
			for (uint32_t q = 0; q < STEER_ROWS; q++) {
				const uint32_t v = s_row[q][t];
				s_row[q][t] = run;
				run += v;
			}
			s_run[t] = run;   // the queue's position after this tile
		}
		__syncthreads();
		steer_one_store<RB, FORM>(f, d, g, x, first, row0, lane, s_row, descs, has_fh, has_mt, has_ti);
		__syncthreads();
		for (uint32_t j = t; j < STEER_ROWS * MOSRX_STEER_BINS; j += MOSRX_STEER_THREADS)
			(&s_row[0][0])[j] = 0;
		__syncthreads();
	}
}

template <uint32_t RB>
static void steer_one_launch(const mosrx_sparams *sp, hipStream_t s)
{
	const dim3 grid(sp->desc ? sp->nb : 1u), block(MOSRX_STEER_THREADS);
	if (!sp->gather)
		hipLaunchKernelGGL((mosrx_steer_one_kernel<RB, STEER_ONE_PLAIN>), grid, block, 0, s, *sp);
	else if (!sp->side)
		hipLaunchKernelGGL((mosrx_steer_one_kernel<RB, STEER_ONE_GATHER>), grid, block, 0, s, *sp);
	else
		hipLaunchKernelGGL((mosrx_steer_one_kernel<RB, STEER_ONE_SIDE>), grid, block, 0, s, *sp);
}

static int gather_ok(const mosrx_sparams *sp)
{
	const mosrx_gdesc *g = &sp->gone;
	const uintptr_t rb = sp->rec_bytes;
	if (sp->desc)
		return sp->gdesc != NULL;
	if (!sp->one.n)
		return 1;
	if (!g->qrec || (((uintptr_t)sp->one.rec | (uintptr_t)g->qrec) & (rb - 1)) || !g->qoff != !g->qlen)
		return 0;
	if (g->qoff && (!g->off || !g->len || (((uintptr_t)g->qoff | (uintptr_t)g->off) & 3) ||
	                (((uintptr_t)g->qlen | (uintptr_t)g->len) & 1)))
		return 0;
	return 1;
}

// The single-batch form's side pairs: both pointers or neither, 4-byte aligned.
static int side_ok(const mosrx_sparams *sp)
{
	const mosrx_xdesc *x = &sp->xone;
	if (!sp->gather)
		return 0;
	if (sp->desc)
		return sp->xdesc != NULL;
	if (!sp->one.n)
		return 1;
	if (!x->fhash != !x->qfhash || !x->match != !x->qmatch || !x->tcpinfo != !x->qtcpinfo)
		return 0;
	return !(((uintptr_t)x->fhash | (uintptr_t)x->qfhash | (uintptr_t)x->match | (uintptr_t)x->qmatch |
	          (uintptr_t)x->tcpinfo | (uintptr_t)x->qtcpinfo) & 3);
}

extern "C" int mosrx_launch_steer(const mosrx_sparams *sp, void *stream)
{
	const hipStream_t s = (hipStream_t)stream;
	if (!sp || (!sp->hist && !sp->fused) || (sp->rec_bytes != 8u && sp->rec_bytes != 16u) || (sp->desc && sp->nb == 0))
		return -EINVAL;
	if (sp->gather && !gather_ok(sp))
		return -EINVAL;
	if (sp->side && !side_ok(sp))
		return -EINVAL;
	if (sp->fused && !sp->desc && sp->one.n > MOSRX_STEER_ONE_MAX)   /* (a table's batches: whoever filled it) */
		return -EINVAL;
	if (sp->total_tiles == 0 && !sp->desc)
		return 0;
	if (sp->fused) {
		if (sp->rec_bytes == 8u)
			steer_one_launch<8u>(sp, s);
		else
			steer_one_launch<16u>(sp, s);
		return hipGetLastError() == hipSuccess ? 0 : -EIO;
	}
	if (sp->total_tiles)
		hipLaunchKernelGGL(mosrx_steer_hist_kernel, dim3(sp->total_tiles), dim3(MOSRX_STEER_THREADS), 0, s, *sp);
	hipLaunchKernelGGL(mosrx_steer_scan_kernel, dim3(sp->desc ? sp->nb : 1u), dim3(SCAN_THREADS), 0, s, *sp);
	if (sp->total_tiles && !sp->gather)
		hipLaunchKernelGGL(mosrx_steer_scatter_kernel, dim3(sp->total_tiles), dim3(MOSRX_STEER_THREADS), 0, s, *sp);
	else if (sp->total_tiles && sp->side && sp->rec_bytes == 8u)
		hipLaunchKernelGGL(mosrx_steer_gather_side_kernel<8u>, dim3(sp->total_tiles), dim3(MOSRX_STEER_THREADS), 0, s, *sp);
	else if (sp->total_tiles && sp->side)
		hipLaunchKernelGGL(mosrx_steer_gather_side_kernel<16u>, dim3(sp->total_tiles), dim3(MOSRX_STEER_THREADS), 0, s, *sp);
	else if (sp->total_tiles && sp->rec_bytes == 8u)
		hipLaunchKernelGGL(mosrx_steer_gather_kernel<8u>, dim3(sp->total_tiles), dim3(MOSRX_STEER_THREADS), 0, s, *sp);
	else if (sp->total_tiles)
		hipLaunchKernelGGL(mosrx_steer_gather_kernel<16u>, dim3(sp->total_tiles), dim3(MOSRX_STEER_THREADS), 0, s, *sp);
	return hipGetLastError() == hipSuccess ? 0 : -EIO;
}
