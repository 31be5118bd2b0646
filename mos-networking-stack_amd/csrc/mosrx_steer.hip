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
	if (!sp || !sp->hist || (sp->rec_bytes != 8u && sp->rec_bytes != 16u) || (sp->desc && sp->nb == 0))
		return -EINVAL;
	if (sp->gather && !gather_ok(sp))
		return -EINVAL;
	if (sp->side && !side_ok(sp))
		return -EINVAL;
	if (sp->total_tiles == 0 && !sp->desc)
		return 0;
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
