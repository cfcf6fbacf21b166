// Polygon regions of interest rasterised into int32 label maps (the definition is with rir_polygon_map_device, include/rir_amd_device.h): the
// reference's scanline fill (DrawPolygon.h:180-398), restated so that every row follows from the rounded vertices alone.  Two kernels:
//
//   polygon_prepare_kernel  a group of 1..64 lanes per (map, polygon): the shifted, rounded vertices, the bounding box clipped to the image
//                           and the vertex count go to the workspace; a polygon that is out of range or outside the image gets an empty box.
//   polygon_fill_kernel     a workgroup per (map, strip of 4 .. PG_ROWS rows, segment of PG_SEG columns), a row per wave at a time.  The wave
//                           fills a row buffer in LDS with the background, then visits in order the polygons whose box holds the row (64
//                           boxes a look) and paints their spans into the buffer; one- and two-point polygons go through the same pass.
//                           The finished row is stored 16 bytes a lane: the buffer starts at the row's offset within 16 bytes, so LDS and
//                           global chunks line up and only a row's head and tail go out as single words.
//
// A polygon's row has two forms, chosen per call by max_pts.  Up to 64 vertices (pg_paint_small, what ROI sets take): several polygons at
// once, each in a group of 4 .. 64 lanes with an edge a lane; one pass computes all their nodes (fp64, as the reference computes them), a
// node's rank among its group's comes from the group's lanes in turn, nothing but the row is in LDS.  More vertices (pg_polygon_row): one
// polygon, 64 edges a pass, the nodes sorted by rank in LDS.  Both apply the first row's rule (equal neighbours dropped in place, an odd count
// paired with the leftover); tests/polygon_cases.py sends the degenerate polygons through both.  What each form and the strip rule buy: DESIGN.md section 7.
//
// A wave owns its rows and its part of the LDS: there are no atomics and no workgroup barriers, every pixel is written once, and nothing
// depends on the order the workgroups run in.  Later polygons overwrite earlier ones because a wave's LDS stores arrive in program order.
#include <algorithm>

#include "polygon_kernels.h"

namespace rir
{
	constexpr int PG_BLOCK = 256;
	constexpr int PG_WAVES = PG_BLOCK / 64;
	constexpr int PG_ROWS = 16;			  // rows of a strip at most
	constexpr int PG_FILL_CHIP = 4096;	  // workgroups that fill the chip
	constexpr int PG_SEG = 1536;		  // columns of a segment: the row buffer of a wave
	constexpr int PG_GRID = 1 << 22;	  // workgroups at most (grid-stride)
	constexpr double PG_LIMIT = 16777216.0; // 2^24: coordinates beyond it, and those that are not finite, draw nothing
	static_assert(PG_SEG % 4 == 0, "segments start on a 16-byte chunk of the row");
	static_assert(PG_WAVES * (PG_SEG + 4 + 2 * (POLYGON_MAX_POINTS + 4)) * 4 <= 64 * 1024, "the workgroup's LDS");

	__device__ __forceinline__ void pg_wave_sync()
	{
		__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
		__builtin_amdgcn_wave_barrier();
		__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
	}

	__device__ __forceinline__ int pg_uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }

	// lanes below this one among those set in mask
	__device__ __forceinline__ int pg_before(unsigned long long mask, int lane) { return __popcll(mask & ((1ull << lane) - 1)); }

	// Workspace of one map, in ints: rows[npoly] (int2: first row, row past the last), cols[npoly] (int2), count[npoly], X[npoly][max_pts],
	// Y[npoly][max_pts]; an even number of ints, so every map's int2 arrays are 8-byte aligned.
	__host__ __device__ inline int64_t pg_map_ints(int npoly, int max_pts)
	{
		const int64_t n = (int64_t)npoly * (5 + 2 * (int64_t)max_pts);
		return n + (n & 1);
	}

	__global__ __launch_bounds__(PG_BLOCK) void polygon_prepare_kernel(const double *__restrict__ xy, const int32_t *__restrict__ npts,
																		const double *__restrict__ shifts, int npoly, int max_pts, int sets_per_map, int w,
																		int h, int group, int64_t items, int32_t *__restrict__ work)
	{
		const int64_t groups = (int64_t)gridDim.x * (PG_BLOCK / group), mine = ((int64_t)blockIdx.x * PG_BLOCK + threadIdx.x) / group;
		const int sub = threadIdx.x % group;
		const int64_t map_ints = pg_map_ints(npoly, max_pts);
		for (int64_t first = 0; first < items; first += groups) // every lane of a wave makes every turn: the shuffles below need them
		{
			const int64_t item = first + mine;
			const bool valid = item < items;
			const int64_t m = valid ? item / npoly : 0;
			const int p = valid ? (int)(item - m * npoly) : 0;
			const int64_t src = (sets_per_map ? m * npoly : 0) + p;
			int n = valid ? npts[src] : 0;
			int bad = n < 0 || n > max_pts;
			n = bad ? 0 : n;
			const double sx = shifts && valid ? shifts[2 * m] : 0.0, sy = shifts && valid ? shifts[2 * m + 1] : 0.0;
			int32_t *wm = work + m * map_ints;
			int32_t *X = wm + 5 * (int64_t)npoly + (int64_t)p * max_pts, *Y = X + (int64_t)npoly * max_pts;
			int xmin = INT32_MAX, xmax = INT32_MIN, ymin = INT32_MAX, ymax = INT32_MIN;
			for (int v = sub; v < n; v += group)
			{
				const double *q = xy + (src * max_pts + v) * 2;
				const double x = shifts ? q[0] + sx : q[0], y = shifts ? q[1] + sy : q[1];
				const bool in = fabs(x) <= PG_LIMIT && fabs(y) <= PG_LIMIT; // false for NaN
				bad |= !in;
				const int xi = in ? (int)round(x) : 0, yi = in ? (int)round(y) : 0;
				X[v] = xi;
				Y[v] = yi;
				xmin = min(xmin, xi), xmax = max(xmax, xi), ymin = min(ymin, yi), ymax = max(ymax, yi);
			}
			for (int d = group >> 1; d > 0; d >>= 1)
			{
				xmin = min(xmin, __shfl_xor(xmin, d)), xmax = max(xmax, __shfl_xor(xmax, d));
				ymin = min(ymin, __shfl_xor(ymin, d)), ymax = max(ymax, __shfl_xor(ymax, d));
				bad |= __shfl_xor(bad, d);
			}
			if (!valid || sub != 0)
				continue;
			int2 rows = make_int2(0, 0), cols = make_int2(0, 0);
			if (!bad && n > 0 && xmax >= 0 && xmin < w && ymax >= 0 && ymin < h) // the box [min, max + 1) meets the image
			{
				rows = make_int2(max(ymin, 0), min(ymax + 1, h));
				cols = make_int2(max(xmin, 0), min(xmax + 1, w));
			}
			reinterpret_cast<int2 *>(wm)[p] = rows;
			reinterpret_cast<int2 *>(wm + 2 * (int64_t)npoly)[p] = cols;
			wm[4 * (int64_t)npoly + p] = rows.y > rows.x ? n : 0;
		}
	}

	// What a wave paints into: its row buffer (column x of the segment at row[x - c0]), the segment's columns and the value.
	struct PgRow
	{
		int *row;
		int c0, c1, lane, value;
		__device__ __forceinline__ void put(int x) const
		{
			if (x >= c0 && x < c1)
				row[x - c0] = value;
		}
		__device__ __forceinline__ void span(int lo, int hi) const // inclusive, by the whole wave
		{
			lo = max(lo, c0), hi = min(hi, c1 - 1);
			for (int x = lo + lane; x <= hi; x += 64)
				row[x - c0] = value;
		}
	};

	// Row y of the two-point form (DrawPolygon.h:196-279): each branch walks from the first point up to the second, which is drawn on its own.
	__device__ __forceinline__ void pg_line_row(const PgRow &r, int x1, int y1, int x2, int y2, int y)
	{
		const int dx = x2 - x1, dy = y2 - y1;
		if (dx == 0)
		{
			if (r.lane == 0)
				r.put(x1);
			return;
		}
		if (dy == 0)
		{
			r.span(min(x1, x2), max(x1, x2));
			return;
		}
		const double a = (double)dy / (double)dx;
		const double ax1 = a * (double)x1;
		const double b = (double)y1 - ax1;
		if (abs(dx) > abs(dy))
		{
			const int lo = max(dx > 0 ? x1 : x2 + 1, r.c0), hi = min(dx > 0 ? x2 - 1 : x1, r.c1 - 1);
			for (int x = lo + r.lane; x <= hi; x += 64)
			{
				const double xa = (double)x * a;
				if ((int)round(xa + b) == y)
					r.row[x - r.c0] = r.value;
			}
		}
		else if (y != y2 && r.lane == 0)
		{
			const double yb = (double)y - b;
			r.put((int)round(yb / a));
		}
		if (y == y2 && r.lane == 0)
			r.put(x2);
	}

	// Does the edge between (.., yi) and the vertex before it (.., yj) cross row y?  first: the first row of the clipped box, where a vertex on
	// the row counts from both sides.
	__device__ __forceinline__ bool pg_crosses(int yi, int yj, int y, bool first)
	{
		return yi != yj && (first ? (yi <= y && yj >= y) || (yj <= y && yi >= y) : (yi < y && yj >= y) || (yj < y && yi >= y));
	}

	// The node of a crossing: the division, the product and the sum are each rounded on their own, as the reference's build rounds them.
	__device__ __forceinline__ int pg_node(int xi, int yi, int xj, int yj, int y)
	{
		const double t = (double)(y - yi) / (double)(yj - yi);
		const double along = t * (double)(xj - xi);
		return (int)round((double)xi + along);
	}

	// Row y of a polygon of n >= 3 vertices (DrawPolygon.h:285-395); first: the first row of its clipped box, [xmin, xmax) the box's columns.
	// A and B hold n + 1 ints each.  The form for any n: 64 edges a pass, the nodes sorted in LDS.
	__device__ __forceinline__ void pg_polygon_row(const PgRow &r, const int32_t *__restrict__ X, const int32_t *__restrict__ Y, int n, int y, bool first,
												   int xmin, int xmax, int *A, int *B)
	{
		int m = 0; // nodes, unsorted in A
		// only the ys decide whether an edge crosses: they are read a pass ahead, a lane's predecessor comes from the lane below it, and the
		// xs are read for the crossings alone
		int before = pg_uniform(Y[n - 1]), ahead = r.lane < n ? Y[r.lane] : 0;
		for (int e0 = 0; e0 < n; e0 += 64)
		{
			const int i = e0 + r.lane, yi = ahead;
			if (e0 + 64 < n)
				ahead = i + 64 < n ? Y[i + 64] : 0;
			int yj = __shfl_up(yi, 1);
			if (r.lane == 0)
				yj = before;
			before = __builtin_amdgcn_readlane(yi, 63);
			const bool cross = i < n && pg_crosses(yi, yj, y, first);
			int node = 0;
			if (cross)
				node = pg_node(X[i], yi, X[i ? i - 1 : n - 1], yj, y);
			const unsigned long long mask = __ballot(cross);
			if (cross)
				A[m + pg_before(mask, r.lane)] = node;
			m += __popcll(mask);
		}
		pg_wave_sync();
		for (int e = r.lane; e < m; e += 64) // rank sort: equal nodes keep their order
		{
			const int v = A[e];
			int rank = 0;
			for (int k = 0; k < m; ++k)
			{
				const int u = A[k];
				rank += u < v || (u == v && k < e);
			}
			B[rank] = v;
		}
		pg_wave_sync();
		const int *nodes = B;
		int count = m, spare = 0; // spare: what an odd count pairs its last node with
		if (first)
		{
			// Equal neighbours are dropped in place in a buffer of n + 1 zeros: the count is at least 1, and the entry after the last
			// kept node is the sorted list's own leftover, or 0.
			int kept = 0;
			for (int e0 = 0; e0 < m; e0 += 64)
			{
				const int e = e0 + r.lane;
				const bool keep = e < m && (e == 0 || B[e] != B[e - 1]);
				const unsigned long long mask = __ballot(keep);
				if (keep)
					A[kept + pg_before(mask, r.lane)] = B[e];
				kept += __popcll(mask);
			}
			if (m == 0)
			{
				if (r.lane == 0)
					A[0] = 0;
				kept = 1;
			}
			spare = kept < m ? pg_uniform(B[kept]) : 0;
			nodes = A;
			count = kept;
			pg_wave_sync();
		}
		for (int i = 0; i < count; i += 2)
		{
			const int a = pg_uniform(nodes[i]), b = i + 1 < count ? pg_uniform(nodes[i + 1]) : spare;
			if (a >= xmax)
				break;
			if (b >= xmin)
				r.span(max(a, xmin), min(b, xmax - 1));
		}
	}

	// The node of the lane that `pick` marks inside the lanes `group` (exactly one; a wave-uniform result).
	__device__ __forceinline__ int pg_pick(int node, bool pick, unsigned long long group)
	{
		const unsigned long long at = __ballot(pick) & group;
		return __builtin_amdgcn_readlane(node, (__ffsll((long long)at) - 1) & 63);
	}

	// The form for sets whose polygons have at most 64 vertices: the next 64 >> log_group polygons of `todo` (the boxes this look found, lane
	// p - p0 holding polygon p's box, count and value) are taken at once, each by a group of 1 << log_group lanes with an edge a lane, so one
	// pass computes the nodes of all of them; a node's rank among its group's comes from the group's lanes in turn.  The spans are then
	// painted group by group, in polygon order.  No LDS but the row.
	__device__ __forceinline__ void pg_paint_small(PgRow &r, unsigned long long &todo, int p0, int log_group, int np, int2 ry, int2 rx, int value,
												   const int32_t *__restrict__ X, const int32_t *__restrict__ Y, int max_pts, int y)
	{
		const int G = 1 << log_group, lane = r.lane, sub = lane & (G - 1), base = lane - sub, slot = lane >> log_group;
		int from = -1, slots = 0;
		for (; slots < (64 >> log_group) && todo; ++slots)
		{
			if (slot == slots)
				from = __ffsll((long long)todo) - 1;
			todo &= todo - 1;
		}
		const int src = max(from, 0);
		int n = __shfl(np, src);
		if (from < 0)
			n = 0;
		const int first_row = __shfl(ry.x, src), xmin = __shfl(rx.x, src), xmax = __shfl(rx.y, src), paint = __shfl(value, src);
		int xi = 0, yi = 0;
		if (sub < n)
		{
			const int32_t at = (p0 + src) * max_pts + sub;
			xi = X[at], yi = Y[at];
		}
		const int prev = sub ? lane - 1 : base + max(n, 1) - 1;
		const int xj = __shfl(xi, prev), yj = __shfl(yi, prev);
		const bool first = y == first_row, cross = sub < n && n >= 3 && pg_crosses(yi, yj, y, first);
		int node = INT32_MAX; // above every node: a lane without a crossing counts for nobody's rank
		if (cross)
			node = pg_node(xi, yi, xj, yj, y);
		int rank = 0;	   // place in the group's sorted nodes, equal nodes in edge order
		bool twin = false; // an equal node before this one: dropped on the first row
		for (int k = 0; k < G; ++k)
		{
			const int other = __shfl(node, base + k);
			rank += other < node || (other == node && k < sub);
			twin |= other == node && k < sub;
		}
		const bool kept = cross && !twin;
		int kept_rank = 0; // place among the nodes the first row keeps
		if (__ballot(first && n >= 3))
		{
			const int mine = kept ? node : INT32_MAX;
			for (int k = 0; k < G; ++k)
				kept_rank += __shfl(mine, base + k) < node;
		}
		const unsigned long long crossing = __ballot(cross), keeping = __ballot(kept);
		for (int s = 0; s < slots; ++s)
		{
			const int b0 = s << log_group, n_s = __builtin_amdgcn_readlane(n, b0), lo = __builtin_amdgcn_readlane(xmin, b0),
					  hi = __builtin_amdgcn_readlane(xmax, b0);
			const int x1 = __builtin_amdgcn_readlane(xi, b0), y1 = __builtin_amdgcn_readlane(yi, b0), x2 = __builtin_amdgcn_readlane(xi, (b0 + 1) & 63),
					  y2 = __builtin_amdgcn_readlane(yi, (b0 + 1) & 63);
			const bool first_s = y == __builtin_amdgcn_readlane(first_row, b0);
			r.value = __builtin_amdgcn_readlane(paint, b0);
			pg_wave_sync(); // the polygon before has left its pixels
			if (n_s == 1)
			{
				if (lane == 0)
					r.put(x1);
			}
			else if (n_s == 2)
				pg_line_row(r, x1, y1, x2, y2, y);
			else if (n_s >= 3)
			{
				const unsigned long long group = (G == 64 ? ~0ull : (1ull << G) - 1) << b0;
				const int m = __popcll(crossing & group);
				int count = m, spare = 0;
				if (first_s) // as in pg_polygon_row: at least one entry, and an odd count pairs its last node with the sorted list's leftover
				{
					count = max(1, __popcll(keeping & group));
					if (count < m)
						spare = pg_pick(node, cross && rank == count, group);
				}
				for (int i = 0; i < count; i += 2)
				{
					int a, b;
					if (first_s)
					{
						a = m ? pg_pick(node, kept && kept_rank == i, group) : 0;
						b = i + 1 < count ? pg_pick(node, kept && kept_rank == i + 1, group) : spare;
					}
					else
					{
						a = pg_pick(node, cross && rank == i, group);
						b = pg_pick(node, cross && rank == i + 1, group);
					}
					if (a >= hi)
						break;
					if (b >= lo)
						r.span(max(a, lo), min(b, hi - 1));
				}
			}
		}
	}

	__global__ __launch_bounds__(PG_BLOCK) void polygon_fill_kernel(const int32_t *__restrict__ work, const int32_t *__restrict__ values, int npoly, int max_pts,
																	 int w, int h, int32_t background, int strips, int segments, int64_t items, int row_ints,
																	 int node_ints, int log_group, int strip_rows, int32_t *__restrict__ dst)
	{
		extern __shared__ __attribute__((aligned(16))) int pg_lds[];
		const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
		int *buf = pg_lds + wave * (row_ints + 2 * node_ints), *A = buf + row_ints, *B = A + node_ints;
		const int64_t map_ints = pg_map_ints(npoly, max_pts);
		for (int64_t item = blockIdx.x; item < items; item += gridDim.x)
		{
			const int seg = (int)(item % segments), strip = (int)(item / segments % strips);
			const int64_t m = item / segments / strips;
			const int c0 = seg * PG_SEG, c1 = min(w, c0 + PG_SEG);
			const int32_t *wm = work + m * map_ints;
			const int2 *rows = reinterpret_cast<const int2 *>(wm), *cols = reinterpret_cast<const int2 *>(wm + 2 * (int64_t)npoly);
			const int32_t *count = wm + 4 * (int64_t)npoly, *X = wm + 5 * (int64_t)npoly, *Y = X + (int64_t)npoly * max_pts;
			for (int y = strip * strip_rows + wave; y < min(h, (strip + 1) * strip_rows); y += PG_WAVES)
			{
				int32_t *out = dst + ((m * h + y) * w + c0);
				const int pad = (int)((uintptr_t)out >> 2 & 3); // the row's first word within its 16 bytes
				for (int i = 4 * lane; i < row_ints; i += 4 * 64)
					*reinterpret_cast<int4 *>(buf + i) = make_int4(background, background, background, background);
				PgRow r{buf + pad, c0, c1, lane, 0};
				for (int p0 = 0; p0 < npoly; p0 += 64)
				{
					const int p = p0 + lane;
					int2 ry = make_int2(0, 0), rx = make_int2(0, 0);
					int np = 0, value = p;
					if (p < npoly)
					{
						ry = rows[p], rx = cols[p], np = count[p];
						if (values)
							value = values[p];
					}
					unsigned long long todo = __ballot(ry.x <= y && y < ry.y && rx.x < c1 && rx.y > c0);
					while (log_group >= 0 && todo)
						pg_paint_small(r, todo, p0, log_group, np, ry, rx, value, X, Y, max_pts, y);
					while (todo)
					{
						const int from = __ffsll((long long)todo) - 1, q = p0 + from;
						todo &= todo - 1;
						const int n = __shfl(np, from), first_row = __shfl(ry.x, from), xmin = __shfl(rx.x, from), xmax = __shfl(rx.y, from);
						const int32_t *Xq = X + (int64_t)q * max_pts, *Yq = Y + (int64_t)q * max_pts;
						r.value = __shfl(value, from);
						pg_wave_sync(); // the polygon before has left its pixels and is done with A and B
						if (n == 1)
						{
							if (lane == 0)
								r.put(Xq[0]);
						}
						else if (n == 2)
							pg_line_row(r, pg_uniform(Xq[0]), pg_uniform(Yq[0]), pg_uniform(Xq[1]), pg_uniform(Yq[1]), y);
						else
							pg_polygon_row(r, Xq, Yq, n, y, y == first_row, xmin, xmax, A, B);
					}
				}
				pg_wave_sync();
				const int width = c1 - c0;
				for (int k = lane; 4 * k < pad + width; k += 64)
				{
					const int4 v = *reinterpret_cast<const int4 *>(buf + 4 * k);
					const int x = 4 * k - pad;
					if (x >= 0 && x + 4 <= width)
						*reinterpret_cast<int4 *>(out + x) = v;
					else
					{
						const int word[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
						for (int j = 0; j < 4; ++j)
							if (x + j >= 0 && x + j < width)
								out[x + j] = word[j];
					}
				}
				pg_wave_sync(); // the row is read before the next one is started
			}
		}
	}

	bool polygon_geometry_ok(int w, int h, int nmaps, int npoly, int max_pts)
	{
		return w >= 1 && h >= 1 && (int64_t)w * h <= POLYGON_MAX_PIXELS && nmaps >= 0 && npoly >= 0 && npoly <= POLYGON_MAX_POLYGONS && max_pts >= 1 &&
			   max_pts <= POLYGON_MAX_POINTS;
	}

	size_t polygon_map_workspace(int w, int h, int nmaps, int npoly, int max_pts)
	{
		if (!polygon_geometry_ok(w, h, nmaps, npoly, max_pts))
			return 0;
		return (size_t)nmaps * (size_t)pg_map_ints(npoly, max_pts) * 4 + 8;
	}

	hipError_t launch_polygon_map(const double *xy, const int32_t *npts, const int32_t *values, int npoly, int max_pts, int nmaps, int sets_per_map,
								  const double *shifts, int w, int h, int32_t background, int32_t *dst, void *work, hipStream_t st)
	{
		if (!polygon_geometry_ok(w, h, nmaps, npoly, max_pts))
			return hipErrorInvalidValue;
		if (nmaps == 0)
			return hipSuccess;
		int32_t *ws = static_cast<int32_t *>(work);
		if (npoly > 0)
		{
			int group = 1;
			while (group < 64 && group < max_pts)
				group *= 2;
			const int64_t items = (int64_t)nmaps * npoly, per_block = PG_BLOCK / group;
			const unsigned grid = (unsigned)std::min<int64_t>(PG_GRID, (items + per_block - 1) / per_block);
			polygon_prepare_kernel<<<grid, PG_BLOCK, 0, st>>>(xy, npts, shifts, npoly, max_pts, sets_per_map, w, h, group, items, ws);
		}
		// a strip of PG_ROWS rows, shorter ones while the workgroups would not fill the chip
		const int segments = (w + PG_SEG - 1) / PG_SEG;
		int strip_rows = PG_ROWS;
		while (strip_rows > PG_WAVES && (int64_t)nmaps * ((h + strip_rows - 1) / strip_rows) * segments < PG_FILL_CHIP)
			strip_rows /= 2;
		const int strips = (h + strip_rows - 1) / strip_rows;
		const int64_t items = (int64_t)nmaps * strips * segments;
		int log_group = -1; // polygons of at most 64 vertices: 4 .. 64 lanes a polygon
		if (max_pts <= 64)
			for (log_group = 2; (1 << log_group) < max_pts; ++log_group)
				;
		const int row_ints = (std::min(w, PG_SEG) + 3 + 3) / 4 * 4, node_ints = log_group >= 0 ? 0 : (max_pts + 1 + 3) / 4 * 4;
		const size_t lds = (size_t)PG_WAVES * (row_ints + 2 * node_ints) * 4;
		polygon_fill_kernel<<<(unsigned)std::min<int64_t>(PG_GRID, items), PG_BLOCK, lds, st>>>(ws, values, npoly, max_pts, w, h, background, strips, segments,
																								items, row_ints, node_ints, log_group, strip_rows, dst);
		return hipGetLastError();
	}
} // namespace rir
