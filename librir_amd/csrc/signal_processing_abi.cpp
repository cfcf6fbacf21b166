// C ABI of the signal_processing half of the hot path.
//
// Two layers, both extern "C":
//   * the reference's own entry points, same names / arguments / return codes
//     (reference src/cpp/signal_processing/signal_processing.h:29-94): host pointers in, host
//     pointers out, synchronous.  They stage through device buffers and call the layer below.
//   * rir_*_device: the same operations on device-resident batches [n][h][w] (no PCIe in the
//     path, asynchronous on the caller's HIP stream) - what pipelines and bench.py use.
// There is no CPU fallback: without a HIP device every entry point logs and returns its error code.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <initializer_list>
#include <map>

#include "distance_kernels.h"
#include "filter_kernels.h"
#include "geometry_kernels.h"
#include "histogram_kernels.h"
#include "label_kernels.h"
#include "local_kernels.h"
#include "morphology_kernels.h"
#include "pixel_kernels.h"
#include "pixel_quantile_kernels.h"
#include "polygon_kernels.h"
#include "quantile_kernels.h"
#include "rank_kernels.h"
#include "reconstruct_kernels.h"
#include "region_kernels.h"
#include "runtime.h"
#include "temporal_kernels.h"
#include "track_kernels.h"

using namespace rir;

namespace
{
	// the caller's stream, taken literally: NULL is HIP's null (legacy default) stream
	hipStream_t as_stream(void *s) { return (hipStream_t)s; }

	struct Span // a byte range of device memory; null or zero bytes: absent
	{
		const void *p;
		size_t bytes;
	};

	// Whether an output overlaps an input or an earlier output; absent spans overlap nothing.
	bool outputs_overlap(std::initializer_list<Span> in, std::initializer_list<Span> out)
	{
		const auto hit = [](const Span &a, const Span &b) {
			return a.p && b.p && a.bytes && b.bytes && (uintptr_t)a.p < (uintptr_t)b.p + b.bytes && (uintptr_t)b.p < (uintptr_t)a.p + a.bytes;
		};
		for (const Span *o = out.begin(); o != out.end(); ++o)
		{
			for (const Span &a : in)
				if (hit(*o, a))
					return true;
			for (const Span *e = out.begin(); e != o; ++e)
				if (hit(*o, *e))
					return true;
		}
		return false;
	}

	// What an extension entry says when it refuses a call: "<its name>: <text>" in the log, -1 to the caller.
	int refuse(const char *who, const std::string &text)
	{
		log_error(std::string(who) + ": " + text);
		return -1;
	}

	// A workspace or a state (`what`) of `have` bytes at p: 8-byte aligned and at least `need`, the bytes that `holds` names; refused otherwise.
	bool workspace_ok(const char *who, const void *p, size_t have, size_t need, const char *what, const char *holds)
	{
		if (have >= need && (uintptr_t)p % 8 == 0)
			return true;
		refuse(who, std::string("the ") + what + " must be 8-byte aligned and hold " + holds + " bytes");
		return false;
	}

	// The percents of a quantile entry into pc; NaN and values outside [0, 1] are refused.
	bool percents_ok(const char *who, const float *percents, int npercents, QuantilePercents &pc)
	{
		for (int j = 0; j < npercents; ++j)
		{
			if (!(percents[j] >= 0.0f && percents[j] <= 1.0f)) // NaN fails both
			{
				refuse(who, "every percent must be in [0, 1]");
				return false;
			}
			pc.p[j] = percents[j];
		}
		return true;
	}

	int strategy_from_string(const char *s)
	{ // signal_processing.cpp:20-41: NULL, "" and "noborder" leave border pixels untouched
		if (!s || std::strlen(s) == 0 || std::strcmp(s, "noborder") == 0)
			return TRANSLATE_UNCHANGED;
		if (std::strcmp(s, "background") == 0)
			return TRANSLATE_CONSTANT;
		if (std::strcmp(s, "wrap") == 0)
			return TRANSLATE_WRAP;
		if (std::strcmp(s, "nearest") == 0)
			return TRANSLATE_NEAREST;
		if (std::strcmp(s, "noborder_source") == 0) // device layer: "noborder" over an implicit copy of the input
			return TRANSLATE_SOURCE;
		return -1;
	}

	int dtype_size(int type)
	{
		switch (type)
		{
		case '?':
		case 'b':
		case 'B':
			return 1;
		case 'h':
		case 'H':
			return 2;
		case 'i':
		case 'I':
		case 'f':
			return 4;
		case 'l':
		case 'L':
		case 'd':
			return 8;
		default:
			return 0;
		}
	}

	// Gaussian table, built exactly as the reference does (signal_processing.cpp:79-99): float exp
	// of a float argument, division by (pi*s) in double, float running sum in x-outer/y-inner
	// order, float normalisation.  Host libm, like the reference.
	int gaussian_radius(float sigma)
	{
		int radius = (int)(sigma * 2);
		return radius < 1 ? 1 : radius;
	}
	std::vector<float> gaussian_table(float sigma, int radius)
	{
		const int kw = 2 * radius + 1;
		std::vector<float> k((size_t)kw * kw);
		const float s = 2.0f * sigma * sigma;
		float sum = 0.0f;
		for (int x = -radius; x <= radius; x++)
			for (int y = -radius; y <= radius; y++)
			{
				const float r = (float)std::sqrt((double)(x * x + y * y));
				const float e = std::exp(-(r * r) / s); // float overload
				const float v = (float)((double)e / (3.14159265358979323846 * (double)s));
				k[x + radius + (y + radius) * kw] = v;
				sum += v;
			}
		for (auto &v : k)
			v /= sum;
		return k;
	}

	// Tables are cached per (device, sigma).  A caller keeps the shared_ptr until its kernel has been QUEUED; freeing a
	// DeviceBuffer is a hipFree, which waits for the work already queued on the device - so an evicted table is never
	// released under a kernel that reads it, whichever thread and stream that kernel runs on.
	typedef std::shared_ptr<DeviceBuffer> GaussTable;
	struct GaussCache
	{
		std::mutex mu;
		std::map<uint64_t, std::pair<GaussTable, uint64_t>> tables; // key = device id << 32 | float bits of sigma -> (table, last use)
		uint64_t tick = 0;
	};
	GaussCache &gauss_cache()
	{
		static GaussCache c;
		return c;
	}
	GaussTable gaussian_table_device(float sigma, int radius)
	{
		uint32_t bits;
		std::memcpy(&bits, &sigma, 4);
		int dev = 0;
		if (!hip_ok(hipGetDevice(&dev), "hipGetDevice"))
			return nullptr;
		const uint64_t key = ((uint64_t)(uint32_t)dev << 32) | bits;
		GaussCache &c = gauss_cache();
		std::lock_guard<std::mutex> g(c.mu);
		auto it = c.tables.find(key);
		if (it != c.tables.end())
		{
			it->second.second = ++c.tick;
			return it->second.first;
		}
		std::vector<float> k = gaussian_table(sigma, radius);
		{ // 1-D factors a[-r..r] of the (separable) table, appended after it: k[dx][dy] ~ a[dx] * a[dy]
			const int kw = 2 * radius + 1;
			const double a0 = std::sqrt((double)k[(size_t)radius * kw + radius]);
			for (int d = 0; d < kw; ++d)
				k.push_back((float)((double)k[(size_t)radius * kw + d] / a0));
		}
		auto buf = std::make_shared<DeviceBuffer>();
		if (!buf->reserve(k.size() * sizeof(float)))
			return nullptr;
		if (!hip_ok(hipMemcpy(buf->ptr, k.data(), k.size() * sizeof(float), hipMemcpyHostToDevice), "gaussian table upload"))
			return nullptr;
		if (c.tables.size() >= 64)
		{ // least recently used entry out (its memory goes when the last holder drops it)
			auto lru = c.tables.begin();
			for (auto i = c.tables.begin(); i != c.tables.end(); ++i)
				if (i->second.second < lru->second.second)
					lru = i;
			c.tables.erase(lru);
		}
		c.tables[key] = std::make_pair(buf, ++c.tick);
		return buf;
	}

	// Scratch for the host-pointer entry points (one call at a time per process; the reference's
	// objects are not re-entrant either).
	struct HostScratch
	{
		std::mutex mu;
		DeviceBuffer a, b, c, d;
		PinnedBuffer h_in, h_out; // page-locked staging of the caller's images
		PinnedBuffer h_tab;		  // label_image: the per-component tables, written by the kernel
	};
	HostScratch &scratch()
	{
		static HostScratch s;
		return s;
	}
	// The caller's images are pageable memory.  Handed to hipMemcpyAsync as they are, the runtime stages them itself, a chunk at a time on
	// the calling thread (measured, one 640x512 image: 70-130 us each way).  Here an image is staged in page-locked memory - the copy cut
	// over the helper threads (host_copy.cpp) - and the KERNEL works on the staging buffers themselves, reading its input and writing its
	// result over the link (profiles/r05_zero_copy_probe.txt: translate of a float image 54 us that way, 89 us with a copy in and a copy out,
	// before the copy calls' own cost): no copy call, one launch, one wait.  RIR_ABI_ZERO_COPY=0: a transfer into / out of device buffers
	// around the kernel, as before.  `slot`: byte offset in the input staging buffer (a call may stage two images).
	// (Round 6, tried and dropped: the image in 2-6 strips of rows - strip j's kernel queued once its rows are staged, the next strip's copy
	// and the previous strip's copy-out under it.  gaussian_filter of a float image: 94 us in one piece, 91 / 89 / 112 / 125 us in 2 / 3 / 4 / 6
	// strips: a launch and an event per strip cost what the overlap of two 14 us copies gains.)
	// -> the address the kernel reads (nullptr on failure)
	// A caller's buffer that lies in page-locked memory of this library (rir_host_alloc: the arrays the Python mirror returns, which are the
	// next call's input) is worked on where it is: no staging copy in, no copy back (round 6: the reference's three-call configs[2] path).
	const void *stage_in(HostScratch &s, DeviceBuffer &d, const void *h_src, size_t bytes, size_t slot, hipStream_t st)
	{
		if (abi_zero_copy() && host_block_contains(h_src, bytes))
			return h_src;
		if (!s.h_in.ptr || s.h_in.cap < slot + bytes)
			return nullptr;
		char *stage = s.h_in.as<char>() + slot;
		host_copy(stage, h_src, bytes);
		if (abi_zero_copy())
			return stage;
		if (!d.reserve(bytes) || !hip_ok(hipMemcpyAsync(d.ptr, stage, bytes, hipMemcpyHostToDevice, st), "H2D"))
			return nullptr;
		return d.ptr;
	}
	// -> the address the kernel writes its result to (nullptr on failure); keep: the caller's buffer holds values the kernel keeps
	// (translate "noborder"), it goes in first
	// in / in_bytes: what the kernel reads (stage_in's answer): a destination that overlaps it is staged, the kernels do not work in place
	void *stage_out(HostScratch &s, DeviceBuffer &d, void *h_dst, size_t bytes, bool keep, hipStream_t st, const void *in = nullptr, size_t in_bytes = 0)
	{
		if (abi_zero_copy() && host_block_contains(h_dst, bytes))
		{
			const char *a = static_cast<const char *>(in), *b = static_cast<const char *>(h_dst);
			if (!in || a + in_bytes <= b || b + bytes <= a)
				return h_dst; // (keep: the caller's values are where the kernel finds them)
		}
		if (!s.h_out.reserve(bytes))
			return nullptr;
		if (keep)
			host_copy(s.h_out.ptr, h_dst, bytes);
		if (abi_zero_copy())
			return s.h_out.ptr;
		if (!d.reserve(bytes) || (keep && !hip_ok(hipMemcpyAsync(d.ptr, s.h_out.ptr, bytes, hipMemcpyHostToDevice, st), "H2D")))
			return nullptr;
		return d.ptr;
	}
	// the call's result (at `from`, what stage_out returned) -> the caller: waits for the stream (the call is synchronous)
	bool hand_out(HostScratch &s, void *h_dst, const void *from, size_t bytes, hipStream_t st)
	{
		if (from == h_dst) // the kernel wrote into the caller's page-locked buffer
			return hip_ok(wait_stream(st), "sync");
		if (from != s.h_out.ptr && !hip_ok(hipMemcpyAsync(s.h_out.ptr, from, bytes, hipMemcpyDeviceToHost, st), "D2H"))
			return false;
		if (!hip_ok(wait_stream(st), "sync"))
			return false;
		host_copy(h_dst, s.h_out.ptr, bytes);
		return true;
	}

	// Bad-pixel object: reference rir::BadPixels (BadPixels.h:14-35) + the loader-side bitmap
	// (IRFileLoader.cpp:704-710).
	struct BadPixelsObject : public Object
	{
		const char *type_name() const override { return "BadPixels"; }
		int width = 0, height = 0;
		int floor_detect = 0;  // Filters.h:157-160
		int floor_correct = 0; // m_median_value, BadPixels.cpp:22-31
		std::vector<int> xy;   // raster order (x,y) pairs
		DeviceBuffer d_xy, d_bitmap;
		DeviceBuffer d_row_start; // [height + 1]: first flagged index of row >= y (the list is in raster order)
		DeviceBuffer d_fix;		  // scratch of the fused filter chain: repaired values, [nframes][count]
		int count() const { return (int)(xy.size() / 2); }
	};

	// double -> int as the reference's casts compile on x86-64 (cvttsd2si): truncation toward zero, and INT_MIN for NaN and for what is
	// out of range.  The squares of deviations beyond 46340 wrap in 32 bits (Filters.h:151-153) and can make the sum negative, the
	// deviation NaN: the casts below then meet NaN, which a plain C++ cast leaves undefined.
	inline int32_t cvtt_i32(double v) { return (v > -2147483649.0 && v < 2147483648.0) ? (int32_t)v : INT32_MIN; }

	// Detector on a device-resident frame.  rows = number of rows taken into account.
	bool detect_bad_pixels(const uint16_t *d_img, int w, int rows, double std_factor, BadPixelsObject &bp, hipStream_t st)
	{
		DeviceBuffer hist, stats, flags;
		const int64_t npx = (int64_t)w * rows;
		if (!hist.reserve(65536 * sizeof(uint32_t)) || !stats.reserve(2 * sizeof(int64_t)) || !flags.reserve((size_t)npx))
			return false;
		if (!hip_ok(launch_histogram(d_img, nullptr, npx, 1, hist.as<uint32_t>(), st), "histogram"))
			return false;
		if (!hip_ok(launch_bad_pixels_stats(hist.as<uint32_t>(), (uint64_t)npx, stats.as<int64_t>(), st), "bad_pixels_stats"))
			return false;
		int64_t h_stats[2];
		if (!hip_ok(hipMemcpyAsync(h_stats, stats.ptr, sizeof(h_stats), hipMemcpyDeviceToHost, st), "stats D2H") ||
			!hip_ok(hipStreamSynchronize(st), "sync"))
			return false;
		// Filters.h:151-160 and BadPixels.cpp:25-31: the sums are exact integers, the rest is the
		// same double sequence as the host code.
		const int median = (int)h_stats[0];
		double sum = (double)h_stats[1];
		sum /= (double)(int)npx;
		sum = std::sqrt(sum);
		const uint16_t thr = (uint16_t)cvtt_i32(sum * std_factor);
		bp.floor_detect = ((uint16_t)median > thr) ? (int)(uint16_t)((uint16_t)median - thr) : 0;
		bp.floor_correct = (int)((uint32_t)median - (uint32_t)cvtt_i32(sum * 2)); // (int arithmetic: wraps like the reference's, NaN -> INT_MIN + median)

		if (!hip_ok(launch_bad_pixels_detect(d_img, w, rows, std_factor, bp.floor_detect, flags.as<uint8_t>(), st), "bad_pixels_detect"))
			return false;
		std::vector<uint8_t> h_flags((size_t)npx);
		if (!hip_ok(hipMemcpyAsync(h_flags.data(), flags.ptr, (size_t)npx, hipMemcpyDeviceToHost, st), "flags D2H") ||
			!hip_ok(hipStreamSynchronize(st), "sync"))
			return false;
		bp.xy.clear();
		for (int y = 0; y < rows; ++y)
			for (int x = 0; x < w; ++x)
				if (h_flags[(size_t)y * w + x])
				{
					bp.xy.push_back(x);
					bp.xy.push_back(y);
				}
		return true;
	}

	bool upload_bad_pixels(BadPixelsObject &bp, hipStream_t st)
	{
		const size_t npx = (size_t)bp.width * bp.height;
		if (!bp.d_xy.reserve(bp.xy.size() * sizeof(int) + 8) || !bp.d_bitmap.reserve(npx))
			return false;
		std::vector<uint8_t> bitmap(npx, 0);
		for (int i = 0; i < bp.count(); ++i)
			bitmap[(size_t)bp.xy[2 * i + 1] * bp.width + bp.xy[2 * i]] = 1;
		if (bp.count() && !hip_ok(hipMemcpyAsync(bp.d_xy.ptr, bp.xy.data(), bp.xy.size() * sizeof(int), hipMemcpyHostToDevice, st), "xy H2D"))
			return false;
		if (!hip_ok(hipMemcpyAsync(bp.d_bitmap.ptr, bitmap.data(), npx, hipMemcpyHostToDevice, st), "bitmap H2D"))
			return false;
		std::vector<int> row_start((size_t)bp.height + 1, bp.count());
		for (int i = bp.count() - 1; i >= 0; --i)
			row_start[bp.xy[2 * i + 1]] = i;
		for (int y = bp.height - 1; y >= 0; --y) // rows without flagged pixels point at the next row's run
			row_start[y] = std::min(row_start[y], row_start[y + 1]);
		if (!bp.d_row_start.reserve(row_start.size() * sizeof(int)) ||
			!hip_ok(hipMemcpyAsync(bp.d_row_start.ptr, row_start.data(), row_start.size() * sizeof(int), hipMemcpyHostToDevice, st), "row_start H2D"))
			return false;
		return hip_ok(hipStreamSynchronize(st), "sync");
	}
} // namespace

// =====================================================================================================
// Device-resident batch layer
// =====================================================================================================

RIR_EXPORT int rir_device_available(void)
{
	int n = 0;
	if (hipGetDeviceCount(&n) != hipSuccess)
	{
		(void)hipGetLastError();
		return 0;
	}
	return n > 0 ? 1 : 0;
}

RIR_EXPORT int rir_stream_synchronize(void *stream)
{
	if (!device_ready())
		return -1;
	return hip_ok(hipStreamSynchronize(as_stream(stream)), "hipStreamSynchronize") ? 0 : -1;
}

RIR_EXPORT int rir_translate_device(int type, const void *d_src, void *d_dst, int w, int h, int nframes, const float *d_offsets,
									int per_frame_offsets, const void *background, const char *strategy, void *stream)
{
	if (!device_ready())
		return -1;
	const int s = strategy_from_string(strategy);
	if (s < 0 || dtype_size(type) == 0 || w <= 0 || h <= 0 || nframes <= 0 || !d_src || !d_dst || !d_offsets || !background)
		return refuse(__func__, "invalid argument");
	return hip_ok(launch_translate(type, d_src, d_dst, background, w, h, nframes, d_offsets, per_frame_offsets, s, as_stream(stream)), "translate") ? 0 : -1;
}

RIR_EXPORT int rir_gaussian_filter_device(const float *d_src, float *d_dst, int w, int h, int nframes, float sigma, void *stream)
{
	if (!device_ready())
		return -1;
	if (w <= 0 || h <= 0 || nframes <= 0 || !d_src || !d_dst || !(sigma > 0))
		return refuse(__func__, "invalid argument");
	const int radius = gaussian_radius(sigma);
	const GaussTable table = gaussian_table_device(sigma, radius); // held until the launch below has been queued
	if (!table)
		return -1;
	const float *d_k = table->as<float>();
	return hip_ok(launch_gaussian(d_src, d_dst, w, h, nframes, d_k, radius, as_stream(stream)), "gaussian_filter") ? 0 : -1;
}

// uint16 frames in, float32 out: gaussian_filter(frame.astype(float32)) without the converted copy in memory (sigma < 2.5).
RIR_EXPORT int rir_gaussian_filter_u16_device(const unsigned short *d_src, float *d_dst, int w, int h, int nframes, float sigma, void *stream)
{
	if (!device_ready())
		return -1;
	if (w <= 0 || h <= 0 || nframes <= 0 || !d_src || !d_dst || !(sigma > 0) || gaussian_radius(sigma) > 4)
		return refuse(__func__, "invalid argument (sigma must be < 2.5 for the uint16 entry)");
	const int radius = gaussian_radius(sigma);
	const GaussTable table = gaussian_table_device(sigma, radius); // held until the launch below has been queued
	if (!table)
		return -1;
	const float *d_k = table->as<float>();
	return hip_ok(launch_gaussian_u16(d_src, d_dst, w, h, nframes, d_k, radius, as_stream(stream)), "gaussian_filter") ? 0 : -1;
}

// float32 frames in, uint16 out: translate(...) followed by the truncating astype(uint16) of the wrapper, in one pass
// (each value is rounded to float first, exactly as the two-step form does).  background: HOST pointer to one uint16.
RIR_EXPORT int rir_translate_f32_u16_device(const float *d_src, unsigned short *d_dst, int w, int h, int nframes, const float *d_offsets,
											int per_frame_offsets, const void *background, const char *strategy, void *stream)
{
	if (!device_ready())
		return -1;
	const int s = strategy_from_string(strategy);
	if (s < 0 || w <= 0 || h <= 0 || nframes <= 0 || !d_src || !d_dst || !d_offsets || !background)
		return refuse(__func__, "invalid argument");
	return hip_ok(launch_translate('F', d_src, d_dst, background, w, h, nframes, d_offsets, per_frame_offsets, s, as_stream(stream)), "translate") ? 0 : -1;
}

// Byte planes of 16-bit frames as the reference hands them to its video codec (h264.cpp:1066-1082) and back (:3016-3051).
// Planes are [nframes][h][linesize] bytes, linesize >= w; d_it (8-bit integration-time image, [nframes][h][w]) may be NULL.
RIR_EXPORT int rir_split_planes_device(const unsigned short *d_img, const unsigned char *d_it, int w, int h, int nframes, int linesize,
									   unsigned char *d_Y, unsigned char *d_U, unsigned char *d_V, void *stream)
{
	if (!device_ready())
		return -1;
	if (!d_img || !d_Y || !d_U || !d_V || w <= 0 || h <= 0 || nframes <= 0 || linesize < w)
		return refuse(__func__, "invalid argument");
	return hip_ok(launch_split_planes(d_img, d_it, w, h, nframes, linesize, d_Y, d_U, d_V, as_stream(stream)), "split_planes") ? 0 : -1;
}
RIR_EXPORT int rir_merge_planes_device(const unsigned char *d_Y, const unsigned char *d_U, const unsigned char *d_V, int linesize, int w, int h,
									   int nframes, unsigned short *d_img, unsigned char *d_it, void *stream)
{
	if (!device_ready())
		return -1;
	if (!d_img || !d_U || !d_V || (d_it && !d_Y) || w <= 0 || h <= 0 || nframes <= 0 || linesize < w)
		return refuse(__func__, "invalid argument");
	return hip_ok(launch_merge_planes(d_Y, d_U, d_V, linesize, w, h, nframes, d_img, d_it, as_stream(stream)), "merge_planes") ? 0 : -1;
}

// result: int32[nframes] on the device.  d_hist: unused (kept in the signature; may be NULL).
RIR_EXPORT int rir_find_median_pixel_device(const unsigned short *d_img, const unsigned char *d_mask, int size, int nframes, float percent,
											int *d_result, unsigned int *d_hist, void *stream)
{
	if (!device_ready())
		return -1;
	if (size <= 0 || nframes <= 0 || !d_img || !d_result)
		return refuse(__func__, "invalid argument");
	(void)d_hist; // the counting happens in LDS, one quarter of the value range at a time: no histogram in memory
	// 65 535 bins, as the reference (Filters.cpp:59)
	return hip_ok(launch_quantile_select(d_img, d_mask, size, nframes, percent, 65535, d_result, as_stream(stream)), "find_median_pixel") ? 0 : -1;
}

RIR_EXPORT int rir_bad_pixels_create_device(const unsigned short *d_first_image, int width, int height, void *stream)
{
	if (!device_ready())
		return 0;
	if (!d_first_image || width <= 0 || height <= 0)
	{
		log_error("rir_bad_pixels_create_device: invalid argument");
		return 0;
	}
	auto bp = std::make_shared<BadPixelsObject>();
	bp->width = width;
	bp->height = height;
	hipStream_t st = as_stream(stream);
	if (!detect_bad_pixels(d_first_image, width, height, 5.0, *bp, st) || !upload_bad_pixels(*bp, st))
		return 0;
	return register_object(bp);
}

RIR_EXPORT int rir_bad_pixels_correct_device(int handle, const unsigned short *d_in, unsigned short *d_out, int nframes, void *stream)
{
	if (!device_ready())
		return -1;
	auto bp = lookup_as<BadPixelsObject>(handle);
	if (!bp || !d_in || !d_out || nframes <= 0)
		return refuse(__func__, "invalid handle or argument");
	return hip_ok(launch_bad_pixels_correct(d_in, d_out, bp->width, bp->height, nframes, bp->d_xy.as<int>(), bp->count(), bp->floor_correct,
											as_stream(stream)),
				  "bad_pixels_correct")
			   ? 0
			   : -1;
}

// The filter chain of BASELINE configs[2] in one pass over the frames: bad_pixels_correct (handle > 0; 0 = skip) ->
// gaussian_filter(sigma) -> translate(offsets, strategy) -> uint16 (truncation, like astype(uint16)).  Bit-identical to
// rir_bad_pixels_correct_device + rir_gaussian_filter_u16_device + rir_translate_f32_u16_device, without the two
// intermediate frames in HBM.  strategy: "nearest", "background" / "constant"; sigma < 2.5; d_src != d_dst.
// background: HOST pointer to one uint16 (may be NULL for "nearest").
RIR_EXPORT int rir_filter_chain_device(int bad_pixels_handle, const unsigned short *d_src, unsigned short *d_dst, int w, int h, int nframes,
									   float sigma, const float *d_offsets, int per_frame_offsets, const void *background, const char *strategy,
									   void *stream)
{
	if (!device_ready())
		return -1;
	const int s = strategy_from_string(strategy);
	if ((s != TRANSLATE_NEAREST && s != TRANSLATE_CONSTANT) || w <= 0 || h <= 0 || nframes <= 0 || !d_src || !d_dst || d_src == d_dst || !d_offsets ||
		!(sigma > 0) || gaussian_radius(sigma) > 4 || (s == TRANSLATE_CONSTANT && !background))
		return refuse(__func__, "invalid argument (strategies: nearest, background; sigma < 2.5; out of place)");
	std::shared_ptr<BadPixelsObject> bp;
	if (bad_pixels_handle > 0)
	{
		bp = lookup_as<BadPixelsObject>(bad_pixels_handle);
		if (!bp || bp->width != w || bp->height != h)
			return refuse(__func__, "invalid bad pixels handle, or created for another image size");
	}
	if (gaussian_reference_order())
	{
		// the reference's own summation order was asked for (runtime.h): the chain as its three steps, still without leaving the device -
		// repair, gaussian_filter as the 2-D sum, translate + truncation - through stream-ordered scratch; the chain's output is then the
		// reference chain's, bit for bit (the fused kernel's separable gaussian differs by +-1 level on < 0.2 % of the pixels)
		hipStream_t st = as_stream(stream);
		const size_t npx = (size_t)w * h * nframes;
		void *d_fixed = nullptr, *d_f32 = nullptr;
		if ((bp && !hip_ok(hipMallocAsync(&d_fixed, npx * 2, st), "hipMallocAsync")) || !hip_ok(hipMallocAsync(&d_f32, npx * 4, st), "hipMallocAsync"))
		{
			if (d_fixed)
				(void)hipFreeAsync(d_fixed, st);
			return -1;
		}
		int r = 0;
		if (bp)
			r = rir_bad_pixels_correct_device(bad_pixels_handle, d_src, static_cast<unsigned short *>(d_fixed), nframes, stream);
		if (r == 0)
			r = rir_gaussian_filter_u16_device(bp ? static_cast<const unsigned short *>(d_fixed) : d_src, static_cast<float *>(d_f32), w, h, nframes, sigma, stream);
		if (r == 0)
			r = rir_translate_f32_u16_device(static_cast<const float *>(d_f32), d_dst, w, h, nframes, d_offsets, per_frame_offsets, background, strategy, stream);
		if (d_fixed)
			(void)hipFreeAsync(d_fixed, st);
		(void)hipFreeAsync(d_f32, st);
		return r;
	}
	const int nbad = bp ? bp->count() : 0;
	if (nbad > 0 && !bp->d_fix.reserve((size_t)nbad * nframes * sizeof(uint32_t)))
		return -1;
	const int radius = gaussian_radius(sigma);
	const GaussTable table = gaussian_table_device(sigma, radius); // held until the launch below has been queued
	if (!table)
		return -1;
	const float *d_k = table->as<float>();
	const uint16_t back = background ? *static_cast<const uint16_t *>(background) : (uint16_t)0;
	return hip_ok(launch_filter_chain(d_src, d_dst, w, h, nframes, bp ? bp->d_xy.as<int>() : nullptr, bp ? bp->d_row_start.as<int>() : nullptr, nbad,
									  bp ? bp->floor_correct : 0, nbad > 0 ? bp->d_fix.as<uint32_t>() : nullptr, d_k, radius, d_offsets,
									  per_frame_offsets, s, back, as_stream(stream)),
				  "filter_chain")
			   ? 0
			   : -1;
}

// info[0] = number of flagged pixels, info[1] = clamp floor (m_median_value), info[2] = detector floor;
// xy (may be NULL) receives up to cap (x,y) pairs in raster order.
RIR_EXPORT int rir_bad_pixels_info(int handle, int *info, int *xy, int cap)
{
	auto bp = lookup_as<BadPixelsObject>(handle);
	if (!bp || !info)
		return -1;
	info[0] = bp->count();
	info[1] = bp->floor_correct;
	info[2] = bp->floor_detect;
	if (xy)
		std::memcpy(xy, bp->xy.data(), sizeof(int) * 2 * (size_t)std::min(cap, bp->count()));
	return 0;
}

// Read-back variant (IRFileLoader::removeBadPixels): in place, first `rows` rows, flagged
// neighbours excluded.  The handle must have been created on a (width x rows) detector window.
RIR_EXPORT int rir_remove_bad_pixels_device(int handle, unsigned short *d_img, int rows, int nframes, void *stream)
{
	if (!device_ready())
		return -1;
	auto bp = lookup_as<BadPixelsObject>(handle);
	if (!bp || !d_img || nframes <= 0 || rows <= 0 || rows > bp->height)
		return refuse(__func__, "invalid handle or argument");
	return hip_ok(launch_remove_bad_pixels(d_img, bp->width, bp->height, rows, nframes, bp->d_xy.as<int>(), bp->count(), bp->d_bitmap.as<uint8_t>(),
										   as_stream(stream)),
				  "remove_bad_pixels")
			   ? 0
			   : -1;
}

// Detector restricted to the first `rows` rows of a (width x height) frame, list expressed in
// full-frame coordinates: what IRFileLoader::setBadPixelsEnabled builds (IRFileLoader.cpp:693-716).
RIR_EXPORT int rir_bad_pixels_create_rows_device(const unsigned short *d_first_image, int width, int height, int rows, void *stream)
{
	if (!device_ready())
		return 0;
	if (!d_first_image || width <= 0 || height <= 0 || rows <= 0 || rows > height)
	{
		log_error("rir_bad_pixels_create_rows_device: invalid argument");
		return 0;
	}
	auto bp = std::make_shared<BadPixelsObject>();
	bp->width = width;
	bp->height = height;
	hipStream_t st = as_stream(stream);
	if (!detect_bad_pixels(d_first_image, width, rows, 5.0, *bp, st) || !upload_bad_pixels(*bp, st))
		return 0;
	return register_object(bp);
}

// Motion removal on read-back (IRFileLoader.cpp:617-627): d_shifts = float pairs (x[pos], y[pos]).
RIR_EXPORT int rir_remove_motion_device(const unsigned short *d_src, unsigned short *d_dst, int w, int h, int rows, int nframes,
										const float *d_shifts, void *stream)
{
	if (!device_ready())
		return -1;
	if (!d_src || !d_dst || d_src == d_dst || w <= 0 || h <= 0 || rows <= 0 || rows > h || nframes <= 0 || !d_shifts)
		return refuse(__func__, "invalid argument");
	return hip_ok(launch_remove_motion(d_src, d_dst, w, h, rows, nframes, d_shifts, as_stream(stream)), "remove_motion") ? 0 : -1;
}

RIR_EXPORT int rir_median_filter_device(const unsigned short *d_src, unsigned short *d_dst, int w, int h, int nframes, void *stream)
{
	if (!device_ready())
		return -1;
	if (!d_src || !d_dst || w < 3 || h < 3 || nframes <= 0)
		return refuse(__func__, "invalid argument (needs w,h >= 3)");
	return hip_ok(launch_median3x3(d_src, d_dst, w, h, nframes, as_stream(stream)), "median_filter") ? 0 : -1;
}

// Temporal median (temporal_kernels.hip).  Every argument is checked here; the source and destination byte ranges may not overlap.
RIR_EXPORT int rir_temporal_median_device(const unsigned short *d_src, unsigned short *d_dst, int w, int h, int nframes, int first, int count, int step,
										  int window, int threshold, int rows, void *stream)
{
	if (!device_ready())
		return -1;
	if (w <= 0 || h <= 0 || nframes <= 0 || window < 1 || window > 63 || window % 2 == 0 || threshold < 0 || threshold > 65535 || rows < 0 || rows > h ||
		step < 1 || count < 0 || first < 0 || first > nframes || (count > 0 && first + (long long)(count - 1) * step > nframes - 1))
		return refuse(__func__, "invalid argument (odd window 1..63, threshold 0..65535, 0 <= rows <= h, outputs inside the stack)");
	if (count == 0)
		return 0;
	const uintptr_t frame = (uintptr_t)w * h * 2, s = (uintptr_t)d_src, d = (uintptr_t)d_dst;
	if (!d_src || !d_dst || (s < d + frame * count && d < s + frame * nframes))
		return refuse(__func__, "null pointer, or the source and destination overlap");
	return hip_ok(launch_temporal_median(d_src, d_dst, w, h, nframes, first, count, step, window, threshold, rows, as_stream(stream)), "temporal_median")
			   ? 0
			   : -1;
}

// The window filters: flat morphology (morphology_kernels.hip) and the spatial rank filters (rank_kernels.hip).  Every argument is checked
// here, before the device is looked for; the byte ranges of the source and the destination may not overlap.
namespace
{
	bool window_type(int type) { return type == 'H' || type == 'B' || type == '?'; }
	bool window_sizes(int size_x, int size_y) { return size_x >= 1 && size_x <= 15 && size_x % 2 == 1 && size_y >= 1 && size_y <= 15 && size_y % 2 == 1; }

	// 0, or what is wrong with the arguments that the window filters share, in the order in which they are tested
	const char *window_filter_args(int type, const void *src, const void *dst, int w, int h, int nframes, int size_x, int size_y, int rows)
	{
		if (!window_type(type))
			return "unknown type (uint16 'H', uint8 'B' or bool '?')";
		if (!window_sizes(size_x, size_y))
			return "size_x and size_y must be odd, 1..15";
		if (w < 1 || h < 1 || nframes < 0 || rows < 0 || rows > h)
			return "invalid shape (w, h >= 1, nframes >= 0, 0 <= rows <= h)";
		if (!src || !dst)
			return "null pointer";
		return nullptr;
	}
	// the same for rir_morphology / rir_morphology_device: the op is tested right after the type
	const char *morphology_args(int type, const void *src, const void *dst, int w, int h, int nframes, int op, int size_x, int size_y, int rows)
	{
		if (window_type(type) && (op < 0 || op >= MORPH_OPS))
			return "unknown op (0 erode, 1 dilate, 2 open, 3 close, 4 tophat, 5 blackhat, 6 gradient)";
		return window_filter_args(type, src, dst, w, h, nframes, size_x, size_y, rows);
	}
	// and for rir_rank_filter / rir_rank_filter_device: the rank is tested right after the sizes
	const char *rank_filter_args(int type, const void *src, const void *dst, int w, int h, int nframes, int rank, int size_x, int size_y, int rows)
	{
		if (window_type(type) && window_sizes(size_x, size_y) && (rank < 0 || rank >= size_x * size_y))
			return "rank must be in 0 .. size_x * size_y - 1";
		return window_filter_args(type, src, dst, w, h, nframes, size_x, size_y, rows);
	}

	// `bad`, or that the byte ranges of the nframes source and destination frames overlap (a host entry works in place: dst == src is allowed)
	const char *or_overlap(const char *bad, int type, const void *src, const void *dst, int w, int h, int nframes, bool same_allowed)
	{
		const uintptr_t bytes = bad ? 0 : (uintptr_t)w * h * (type == 'H' ? 2 : 1) * nframes, s = (uintptr_t)src, d = (uintptr_t)dst;
		if (bad || (same_allowed && s == d) || !(s < d + bytes && d < s + bytes))
			return bad;
		return same_allowed ? "the source and the destination overlap (dst == src is allowed)" : "the source and the destination overlap";
	}

	// A device entry of a window filter, `bad` being what its check found: refused before the device is looked for; no frames is no work.
	template <class Launch>
	int window_filter_device(const char *who, const char *what, const char *bad, int type, const void *d_src, void *d_dst, int w, int h, int nframes,
							 Launch launch)
	{
		bad = or_overlap(bad, type, d_src, d_dst, w, h, nframes, false);
		if (bad)
			return refuse(who, bad);
		if (nframes == 0)
			return 0;
		if (!device_ready())
			return -1;
		return hip_ok(launch(), what) ? 0 : -1;
	}
} // namespace

RIR_EXPORT int rir_morphology_device(int type, const void *d_src, void *d_dst, int w, int h, int nframes, int op, int size_x, int size_y, int rows,
									 void *stream)
{
	return window_filter_device(__func__, "morphology", morphology_args(type, d_src, d_dst, w, h, nframes, op, size_x, size_y, rows), type, d_src, d_dst, w,
								h, nframes, [=] { return launch_morphology(type, d_src, d_dst, w, h, nframes, op, size_x, size_y, rows, as_stream(stream)); });
}

RIR_EXPORT int rir_rank_filter_device(int type, const void *d_src, void *d_dst, int w, int h, int nframes, int rank, int size_x, int size_y, int rows,
									  void *stream)
{
	return window_filter_device(__func__, "rank_filter", rank_filter_args(type, d_src, d_dst, w, h, nframes, rank, size_x, size_y, rows), type, d_src, d_dst,
								w, h, nframes, [=] { return launch_rank_filter(type, d_src, d_dst, w, h, nframes, rank, size_x, size_y, rows, as_stream(stream)); });
}

// The local window statistics (local_kernels.hip).  Every argument is checked here, before the device is looked for, in the order of
// window_filter_args with the entry's own conditions at their places; no output may overlap the input or another output.
namespace
{
	// 0, or what is wrong with the arguments of rir_local_stats / rir_local_stats_device: the outputs are tested after the shape and the source
	const char *local_stats_args(int type, const void *src, int w, int h, int nframes, int size_x, int size_y, int rows, const int *sum, const long long *sumsq,
								 const void *mean)
	{
		if (const char *bad = window_filter_args(type, src, src, w, h, nframes, size_x, size_y, rows))
			return bad;
		if (!sum && !sumsq && !mean)
			return "no output asked for (the sum, the sum of squares and the mean are all null)";
		const size_t npx = (size_t)w * h * nframes;
		if (outputs_overlap({{src, npx * (type == 'H' ? 2 : 1)}}, {{sum, npx * 4}, {sumsq, npx * 8}, {mean, npx * (type == 'H' ? 2 : 1)}}))
			return "an output overlaps the input or another output";
		return nullptr;
	}
	// the same for rir_local_threshold / rir_local_threshold_device: the rule's parameters are tested right after the sizes
	const char *local_threshold_args(int type, const void *src, const void *mask, int w, int h, int nframes, int size_x, int size_y, int rows, int k_num,
									 int k_den, int delta, int polarity)
	{
		if (window_type(type) && window_sizes(size_x, size_y))
		{
			if (k_num < 0 || k_num > LOCAL_K_NUM_MAX || k_den < 1 || k_den > LOCAL_K_DEN_MAX)
				return "k_num must be in 0..255 and k_den in 1..64";
			if (delta < -LOCAL_DELTA_MAX || delta > LOCAL_DELTA_MAX)
				return "delta must be in -65535..65535";
			if (polarity < 0 || polarity >= LOCAL_POLARITIES)
				return "unknown polarity (0 above, 1 below, 2 both)";
		}
		if (const char *bad = window_filter_args(type, src, mask, w, h, nframes, size_x, size_y, rows))
			return bad;
		const size_t npx = (size_t)w * h * nframes;
		if (outputs_overlap({{src, npx * (type == 'H' ? 2 : 1)}}, {{mask, npx}}))
			return "the mask overlaps the input";
		return nullptr;
	}
} // namespace

RIR_EXPORT int rir_local_stats_device(int type, const void *d_src, int w, int h, int nframes, int size_x, int size_y, int rows, int *d_sum, long long *d_sumsq,
									  void *d_mean, void *stream)
{
	if (const char *bad = local_stats_args(type, d_src, w, h, nframes, size_x, size_y, rows, d_sum, d_sumsq, d_mean))
		return refuse(__func__, bad);
	if (nframes == 0)
		return 0;
	if (!device_ready())
		return -1;
	return hip_ok(launch_local_stats(type, d_src, w, h, nframes, size_x, size_y, rows, d_sum, (int64_t *)d_sumsq, d_mean, as_stream(stream)), "local_stats")
			   ? 0
			   : -1;
}

RIR_EXPORT int rir_local_threshold_device(int type, const void *d_src, unsigned char *d_mask, int w, int h, int nframes, int size_x, int size_y, int rows,
										  int k_num, int k_den, int delta, int polarity, void *stream)
{
	if (const char *bad = local_threshold_args(type, d_src, d_mask, w, h, nframes, size_x, size_y, rows, k_num, k_den, delta, polarity))
		return refuse(__func__, bad);
	if (nframes == 0)
		return 0;
	if (!device_ready())
		return -1;
	return hip_ok(launch_local_threshold(type, d_src, d_mask, w, h, nframes, size_x, size_y, rows, k_num, k_den, delta, polarity, as_stream(stream)),
				  "local_threshold")
			   ? 0
			   : -1;
}

// The exact Euclidean distance transform (distance_kernels.hip).  Every argument is checked here, before the device is looked for; no output
// (workspace included) may overlap the input or another output.
namespace
{
	constexpr size_t DISTANCE_WORK_BYTES = (size_t)256 << 20; // what the workspace query asks for at most, or one frame's need

	int distance_cell_bytes(int type) { return type == '?' || type == 'B' ? 1 : type == 'H' ? 2 : type == 'i' ? 4 : 0; }
	bool distance_geometry(int w, int h, int nframes) { return w >= 1 && w <= DISTANCE_MAX_SIDE && h >= 1 && h <= DISTANCE_MAX_SIDE && nframes >= 0; }

	// 0, or what is wrong with the arguments that rir_distance_transform and rir_distance_transform_device share, in the order of the tests
	const char *distance_transform_args(int type, const void *src, int w, int h, int nframes, int background, int border, int rows, const int *dist2,
										const int *index)
	{
		const int cell = distance_cell_bytes(type);
		if (!cell)
			return "unknown type (bool '?', uint8 'B', uint16 'H' or int32 'i')";
		if (cell < 4 && (background < 0 || background > (type == '?' ? 1 : type == 'B' ? 255 : 65535)))
			return "background outside the range of the type";
		if (border != 0 && border != 1)
			return "border must be 0 or 1";
		if (!distance_geometry(w, h, nframes) || rows < 0 || rows > h)
			return "invalid shape (1 <= w, h <= 16384, nframes >= 0, 0 <= rows <= h)";
		if (!src || !dist2)
			return "null pointer (only the index may be null)";
		const size_t npx = (size_t)w * h * nframes;
		if (outputs_overlap({{src, npx * cell}}, {{dist2, npx * 4}, {index, npx * 4}}))
			return "an output overlaps the input or the other output";
		return nullptr;
	}
} // namespace

RIR_EXPORT size_t rir_distance_transform_workspace_bytes(int w, int h, int nframes, int want_indices)
{
	if (!distance_geometry(w, h, nframes) || (want_indices != 0 && want_indices != 1))
		return 0;
	const size_t B = distance_frame_bytes(w, h); // (the same with and without indices: the index comes from what the passes keep anyway)
	return B * std::min<size_t>((size_t)std::max(nframes, 1), std::max<size_t>(1, DISTANCE_WORK_BYTES / B));
}

RIR_EXPORT int rir_distance_transform_device(int type, const void *d_src, int w, int h, int nframes, int background, int border, int rows, int *d_dist2,
											 int *d_index, void *d_work, size_t work_bytes, void *stream)
{
	if (const char *bad = distance_transform_args(type, d_src, w, h, nframes, background, border, rows, d_dist2, d_index))
		return refuse(__func__, bad);
	const size_t B = distance_frame_bytes(w, h);
	if (!d_work)
		return refuse(__func__, "null pointer (the workspace)");
	if (!workspace_ok(__func__, d_work, work_bytes, B, "workspace", "one frame's share of rir_distance_transform_workspace_bytes()"))
		return -1;
	const size_t npx = (size_t)w * h * nframes, used = B * std::min<size_t>((size_t)nframes, work_bytes / B);
	if (outputs_overlap({{d_src, npx * distance_cell_bytes(type)}, {d_dist2, npx * 4}, {d_index, npx * 4}}, {{d_work, used}}))
		return refuse(__func__, "the workspace overlaps the input or an output");
	if (nframes == 0)
		return 0;
	if (!device_ready())
		return -1;
	return hip_ok(launch_distance_transform(type, d_src, w, h, nframes, background, border, rows, d_dist2, d_index, d_work, work_bytes, as_stream(stream)),
				  "distance_transform")
			   ? 0
			   : -1;
}

// Grey-level morphological reconstruction (reconstruct_kernels.hip).  Every argument is checked here, before the device is looked for; the
// destination (and the workspace) may overlap neither input, the marker may be the mask.
namespace
{
	constexpr size_t RECONSTRUCT_WORK_BYTES = (size_t)256 << 20; // what the workspace query asks for at most

	bool reconstruct_geometry(int w, int h, int nframes) { return w >= 1 && h >= 1 && (int64_t)w * h <= 0x7fffffff && nframes >= 0; }

	// 0, or what is wrong with the arguments that rir_reconstruct and rir_reconstruct_device share, in the order of the tests
	const char *reconstruct_args(int type, const void *mask, const void *marker, const void *dst, int w, int h, int nframes, int method, int connectivity,
								 int marker_mode, int param, int output, int rows)
	{
		if (!window_type(type))
			return "unknown type (uint16 'H', uint8 'B' or bool '?')";
		if (method != 0 && method != 1)
			return "unknown method (0 dilation, 1 erosion)";
		if (connectivity != 4 && connectivity != 8)
			return "connectivity must be 4 or 8";
		if (marker_mode < 0 || marker_mode >= RECONSTRUCT_MARKERS)
			return "unknown marker mode (0 explicit, 1 the mask shifted by param, 2 the mask on the border)";
		if (output != 0 && output != 1)
			return "unknown output (0 the reconstruction, 1 its difference to the mask)";
		if (param < 0 || param > (type == 'H' ? 65535 : type == 'B' ? 255 : 1))
			return "param outside the range of the type";
		if (!reconstruct_geometry(w, h, nframes) || rows < 0 || rows > h)
			return "invalid shape (w, h >= 1, w * h < 2^31, nframes >= 0, 0 <= rows <= h)";
		if (!mask || !dst)
			return "null pointer";
		if ((marker_mode == 0) != (marker != nullptr))
			return "a marker stack goes with marker mode 0, and with no other";
		const size_t bytes = (size_t)w * h * nframes * (type == 'H' ? 2 : 1);
		if (outputs_overlap({{mask, bytes}, {marker, bytes}}, {{dst, bytes}}))
			return "the destination overlaps the mask or the marker";
		return nullptr;
	}
} // namespace

RIR_EXPORT size_t rir_reconstruct_workspace_bytes(int type, int w, int h, int nframes)
{
	if (!window_type(type) || !reconstruct_geometry(w, h, nframes))
		return 0;
	return RECONSTRUCT_FRAME_BYTES * std::min<size_t>((size_t)std::max(nframes, 1), RECONSTRUCT_WORK_BYTES / RECONSTRUCT_FRAME_BYTES);
}

RIR_EXPORT int rir_reconstruct_device(int type, const void *d_mask, const void *d_marker, void *d_dst, int w, int h, int nframes, int method,
									  int connectivity, int marker_mode, int param, int output, int rows, void *d_work, size_t work_bytes, int *rounds,
									  void *stream)
{
	if (const char *bad = reconstruct_args(type, d_mask, d_marker, d_dst, w, h, nframes, method, connectivity, marker_mode, param, output, rows))
		return refuse(__func__, bad);
	if (!d_work)
		return refuse(__func__, "null pointer (the workspace)");
	if (!workspace_ok(__func__, d_work, work_bytes, RECONSTRUCT_FRAME_BYTES, "workspace", "one frame's share of rir_reconstruct_workspace_bytes()"))
		return -1;
	const size_t bytes = (size_t)w * h * nframes * (type == 'H' ? 2 : 1);
	const size_t used = RECONSTRUCT_FRAME_BYTES * std::min<size_t>((size_t)nframes, work_bytes / RECONSTRUCT_FRAME_BYTES);
	if (outputs_overlap({{d_mask, bytes}, {d_marker, bytes}, {d_dst, bytes}}, {{d_work, used}}))
		return refuse(__func__, "the workspace overlaps an input or the destination");
	if (rounds)
		*rounds = 0;
	if (nframes == 0)
		return 0;
	if (!device_ready())
		return -1;
	thread_local PinnedBuffer h_flags; // the flags of a round, as the host reads them
	if (!h_flags.reserve(sizeof(int) * (size_t)reconstruct_group_frames(nframes, work_bytes)))
		return -1;
	int took = 0;
	bool converged = true;
	if (!hip_ok(launch_reconstruct(type, d_mask, d_marker, d_dst, w, h, nframes, method, connectivity, marker_mode, param, output, rows, d_work, work_bytes,
								   h_flags.as<int>(), &took, &converged, as_stream(stream)),
				"reconstruct"))
		return -1;
	if (rounds)
		*rounds = took;
	return converged ? 0 : refuse(__func__, "did not converge within w * rows + 2 rounds");
}

// Per-region statistics (region_kernels.hip).  Every argument is checked here; no output (workspace included) may overlap an input or
// another output.
namespace
{
	bool region_stats_args(int w, int h, int nframes, int labels_per_frame, int nregions)
	{
		return w > 0 && h > 0 && (long long)w * h < (1ll << 31) && nframes >= 0 && (labels_per_frame == 0 || labels_per_frame == 1) && nregions >= 1 &&
			   nregions <= (1 << 24);
	}
} // namespace

RIR_EXPORT size_t rir_region_stats_workspace_bytes(int w, int h, int nframes, int labels_per_frame, int nregions)
{
	if (!region_stats_args(w, h, nframes, labels_per_frame, nregions))
		return 0;
	return region_stats_workspace((int64_t)w * h, nframes, nregions);
}

RIR_EXPORT int rir_region_stats_device(const unsigned short *d_frames, const int *d_labels, int w, int h, int nframes, int labels_per_frame, int nregions,
									   int *d_count, long long *d_sum, long long *d_sumsq, int *d_min, int *d_max, int *d_argmin, int *d_argmax,
									   void *d_work, size_t work_bytes, void *stream)
{
	if (!device_ready())
		return -1;
	if (!region_stats_args(w, h, nframes, labels_per_frame, nregions))
		return refuse(__func__, "invalid argument (w, h >= 1 with w * h < 2^31, nframes >= 0, labels_per_frame 0 or 1, 1 <= nregions <= 2^24)");
	if (nframes == 0)
		return 0;
	const size_t npx = (size_t)w * h, cells = (size_t)nframes * nregions, need = region_stats_workspace((int64_t)npx, nframes, nregions);
	if (!d_frames || !d_labels || !d_count || !d_sum || !d_sumsq || !d_min || !d_max || !d_argmin || !d_argmax || !d_work)
		return refuse(__func__, "null pointer");
	if (!workspace_ok(__func__, d_work, work_bytes, need, "workspace", "rir_region_stats_workspace_bytes()"))
		return -1;
	if (outputs_overlap({{d_frames, npx * nframes * 2}, {d_labels, npx * (labels_per_frame ? nframes : 1) * 4}},
						{{d_count, cells * 4}, {d_sum, cells * 8}, {d_sumsq, cells * 8}, {d_min, cells * 4}, {d_max, cells * 4}, {d_argmin, cells * 4},
						 {d_argmax, cells * 4}, {d_work, need}}))
		return refuse(__func__, "an output or the workspace overlaps an input or another output");
	return hip_ok(launch_region_stats(d_frames, d_labels, (int64_t)npx, nframes, labels_per_frame, nregions, d_count, (int64_t *)d_sum, (int64_t *)d_sumsq,
									  d_min, d_max, d_argmin, d_argmax, d_work, as_stream(stream)),
				  "region_stats")
			   ? 0
			   : -1;
}

// Per-region geometry (geometry_kernels.hip).  Every argument is checked here; no output (workspace included) may overlap an input or
// another output.
namespace
{
	// region_stats' arguments with both sides at most 32768 (every sum then stays below 2^62); without weights nframes counts label maps
	bool region_geometry_args(int w, int h, int nframes, int labels_per_frame, int nregions, int weighted)
	{
		return region_stats_args(w, h, nframes, labels_per_frame, nregions) && w <= 32768 && h <= 32768 && (weighted == 0 || weighted == 1) &&
			   (weighted || labels_per_frame || nframes <= 1);
	}
	const char *const REGION_GEOMETRY_ARGS = "invalid argument (1 <= w, h <= 32768 with w * h < 2^31, nframes >= 0, labels_per_frame 0 or 1, "
											 "1 <= nregions <= 2^24; without frames labels_per_frame 1 or nframes <= 1)";
} // namespace

RIR_EXPORT size_t rir_region_geometry_workspace_bytes(int w, int h, int nframes, int labels_per_frame, int nregions, int weighted)
{
	return region_geometry_args(w, h, nframes, labels_per_frame, nregions, weighted) ? GEOMETRY_WORK_BYTES : 0;
}

RIR_EXPORT int rir_region_geometry_device(const int *d_labels, const unsigned short *d_frames, int w, int h, int nframes, int labels_per_frame, int nregions,
										  int *d_count, int *d_bbox, long long *d_moments, long long *d_weighted, void *d_work, size_t work_bytes,
										  void *stream)
{
	if (!device_ready())
		return -1;
	if (!region_geometry_args(w, h, nframes, labels_per_frame, nregions, d_frames != nullptr))
		return refuse(__func__, REGION_GEOMETRY_ARGS);
	if (nframes == 0)
		return 0;
	if (!d_labels || !d_count || !d_bbox || !d_moments || !d_work || (d_frames != nullptr) != (d_weighted != nullptr))
		return refuse(__func__, "null pointer (d_weighted is null exactly when d_frames is)");
	if (!workspace_ok(__func__, d_work, work_bytes, GEOMETRY_WORK_BYTES, "workspace", "rir_region_geometry_workspace_bytes()"))
		return -1;
	const size_t npx = (size_t)w * h, cells = (size_t)nframes * nregions;
	if (outputs_overlap({{d_labels, npx * (labels_per_frame ? nframes : 1) * 4}, {d_frames, npx * nframes * 2}},
						{{d_count, cells * 4}, {d_bbox, cells * 16}, {d_moments, cells * 40}, {d_work, GEOMETRY_WORK_BYTES}, {d_weighted, cells * 24}}))
		return refuse(__func__, "an output or the workspace overlaps an input or another output");
	return hip_ok(launch_region_geometry(d_labels, d_frames, w, h, nframes, labels_per_frame, nregions, d_count, d_bbox, (int64_t *)d_moments,
										 (int64_t *)d_weighted, as_stream(stream)),
				  "region_geometry")
			   ? 0
			   : -1;
}

// Per-region quantiles (quantile_kernels.hip).  Every argument is checked here; no output (workspace included) may overlap an input or
// another output.
namespace
{
	bool region_quantiles_args(int w, int h, int nframes, int labels_per_frame, int nregions, int npercents)
	{
		return region_stats_args(w, h, nframes, labels_per_frame, nregions) && nregions <= QUANTILE_MAX_REGIONS && npercents >= 1 &&
			   npercents <= QUANTILE_MAX_PERCENTS;
	}
	constexpr size_t QUANTILE_WORK_BYTES = (size_t)256 << 20; // what the workspace query asks for at most, or one frame's need
} // namespace

RIR_EXPORT size_t rir_region_quantiles_workspace_bytes(int w, int h, int nframes, int labels_per_frame, int nregions, int npercents)
{
	if (!region_quantiles_args(w, h, nframes, labels_per_frame, nregions, npercents))
		return 0;
	const size_t B = region_quantiles_frame_bytes(nregions, npercents);
	return B * std::min<size_t>((size_t)std::max(nframes, 1), std::max<size_t>(1, QUANTILE_WORK_BYTES / B));
}

RIR_EXPORT int rir_region_quantiles_device(const unsigned short *d_frames, const int *d_labels, int w, int h, int nframes, int labels_per_frame,
											int nregions, const float *percents, int npercents, int *d_count, int *d_values, void *d_work,
											size_t work_bytes, void *stream)
{
	if (!device_ready())
		return -1;
	if (!region_quantiles_args(w, h, nframes, labels_per_frame, nregions, npercents))
		return refuse(__func__, "invalid argument (w, h >= 1 with w * h < 2^31, nframes >= 0, labels_per_frame 0 or 1, 1 <= nregions <= 65536, "
								"1 <= npercents <= 8)");
	if (!d_frames || !d_labels || !percents || !d_count || !d_values || !d_work)
		return refuse(__func__, "null pointer");
	QuantilePercents pc{};
	if (!percents_ok(__func__, percents, npercents, pc))
		return -1;
	if (nframes == 0)
		return 0;
	const size_t npx = (size_t)w * h, cells = (size_t)nframes * nregions, B = region_quantiles_frame_bytes(nregions, npercents);
	if (!workspace_ok(__func__, d_work, work_bytes, B, "workspace", "one frame's share of rir_region_quantiles_workspace_bytes()"))
		return -1;
	const size_t used = B * std::min<size_t>((size_t)nframes, work_bytes / B);
	if (outputs_overlap({{d_frames, npx * nframes * 2}, {d_labels, npx * (labels_per_frame ? nframes : 1) * 4}},
						{{d_count, cells * 4}, {d_values, cells * npercents * 4}, {d_work, used}}))
		return refuse(__func__, "an output or the workspace overlaps an input or another output");
	return hip_ok(launch_region_quantiles(d_frames, d_labels, (int64_t)npx, nframes, labels_per_frame, nregions, pc, npercents, d_count, d_values, d_work,
										  work_bytes, as_stream(stream)),
				  "region_quantiles")
			   ? 0
			   : -1;
}

// Per-region histograms (histogram_kernels.hip).  Every argument is checked here, before the device is looked for; no output (workspace
// included) may overlap an input or another output.
namespace
{
	const char *const REGION_HISTOGRAM_ARGS = "invalid argument (w, h >= 1 with w * h < 2^31, 0 <= rows <= h, nframes >= 0, labels_per_frame 0 or 1, "
											  "1 <= nregions <= 65536, 0 <= lo <= 65535, 1 <= width <= 65536, 1 <= nbins <= 65536, "
											  "nregions * nbins <= 2^24; without labels nregions 1 and labels_per_frame 0)";
	bool region_histogram_args(bool labelled, int w, int h, int rows, int nframes, int labels_per_frame, int nregions, int lo, int width, int nbins)
	{
		return region_stats_args(w, h, nframes, labels_per_frame, nregions) && rows >= 0 && rows <= h && nregions <= HISTOGRAM_MAX_REGIONS && lo >= 0 &&
			   lo <= 65535 && width >= 1 && width <= 65536 && nbins >= 1 && nbins <= HISTOGRAM_MAX_BINS &&
			   (long long)nregions * nbins <= HISTOGRAM_MAX_CELLS && (labelled || (nregions == 1 && labels_per_frame == 0));
	}
} // namespace

RIR_EXPORT size_t rir_region_histogram_workspace_bytes(int w, int h, int rows, int nframes, int labels_per_frame, int nregions, int nbins)
{
	return region_histogram_args(true, w, h, rows, nframes, labels_per_frame, nregions, 0, 1, nbins) ? HISTOGRAM_WORK_BYTES : 0;
}

RIR_EXPORT int rir_region_histogram_device(const unsigned short *d_frames, const int *d_labels, int w, int h, int rows, int nframes, int labels_per_frame,
											int nregions, int lo, int width, int nbins, int *d_count, int *d_hist, int *d_outside, void *d_work,
											size_t work_bytes, void *stream)
{
	if (!region_histogram_args(d_labels != nullptr, w, h, rows, nframes, labels_per_frame, nregions, lo, width, nbins))
		return refuse(__func__, REGION_HISTOGRAM_ARGS);
	if (!d_frames || !d_hist || !d_work)
		return refuse(__func__, "null pointer (only d_labels, d_count and d_outside may be null)");
	if (!workspace_ok(__func__, d_work, work_bytes, HISTOGRAM_WORK_BYTES, "workspace", "rir_region_histogram_workspace_bytes()"))
		return -1;
	const size_t npx = (size_t)w * h, cells = (size_t)nframes * nregions;
	if (outputs_overlap({{d_frames, npx * nframes * 2}, {d_labels, npx * (labels_per_frame ? nframes : 1) * 4}},
						{{d_count, cells * 4}, {d_hist, cells * nbins * 4}, {d_outside, cells * 8}, {d_work, HISTOGRAM_WORK_BYTES}}))
		return refuse(__func__, "an output or the workspace overlaps an input or another output");
	if (nframes == 0)
		return 0;
	if (!device_ready())
		return -1;
	return hip_ok(launch_region_histogram(d_frames, d_labels, (int64_t)npx, (int64_t)rows * w, nframes, labels_per_frame, nregions, lo, width, nbins,
										  d_count, d_hist, d_outside, as_stream(stream)),
				  "region_histogram")
			   ? 0
			   : -1;
}

// Per-pixel statistics over time (pixel_kernels.hip).  Every argument is checked here; no output (workspace included) may overlap the input
// or another output.
namespace
{
	bool pixel_stats_args(int w, int h, int nframes) { return w > 0 && h > 0 && (long long)w * h < (1ll << 31) && nframes >= 0; }
} // namespace

RIR_EXPORT size_t rir_pixel_stats_workspace_bytes(int w, int h, int nframes)
{
	if (!pixel_stats_args(w, h, nframes))
		return 0;
	return pixel_stats_workspace((int64_t)w * h, nframes);
}

RIR_EXPORT int rir_pixel_stats_device(const unsigned short *d_frames, int w, int h, int nframes, int t0, int accumulate, long long *d_sum,
									  long long *d_sumsq, int *d_min, int *d_max, int *d_argmin, int *d_argmax, void *d_work, size_t work_bytes,
									  void *stream)
{
	if (!device_ready())
		return -1;
	if (!pixel_stats_args(w, h, nframes) || t0 < 0 || (long long)t0 + nframes > 2147483647ll || (accumulate != 0 && accumulate != 1))
		return refuse(__func__, "invalid argument (w, h >= 1 with w * h < 2^31, nframes >= 0, t0 >= 0 with t0 + nframes <= 2^31 - 1, accumulate 0 or 1)");
	if (nframes == 0)
		return 0;
	const bool sums = d_sum || d_sumsq, extremes = d_min || d_max || d_argmin || d_argmax;
	if ((sums && (!d_sum || !d_sumsq)) || (extremes && (!d_min || !d_max || !d_argmin || !d_argmax)) || (!sums && !extremes))
		return refuse(__func__, "a group of outputs (sum, sumsq / min, max, argmin, argmax) is all given or all null, and one is given");
	if (!d_frames || !d_work)
		return refuse(__func__, "null pointer");
	const size_t npx = (size_t)w * h, need = pixel_stats_workspace((int64_t)npx, nframes);
	if (!workspace_ok(__func__, d_work, work_bytes, need, "workspace", "rir_pixel_stats_workspace_bytes()"))
		return -1;
	if (outputs_overlap({{d_frames, npx * nframes * 2}}, {{d_sum, npx * 8}, {d_sumsq, npx * 8}, {d_min, npx * 4}, {d_max, npx * 4}, {d_argmin, npx * 4},
															{d_argmax, npx * 4}, {d_work, need}})) // the group not asked for is null: absent
		return refuse(__func__, "an output or the workspace overlaps the input or another output");
	return hip_ok(launch_pixel_stats(d_frames, (int64_t)npx, nframes, t0, accumulate, (int64_t *)d_sum, (int64_t *)d_sumsq, d_min, d_max, d_argmin,
									 d_argmax, d_work, as_stream(stream)),
				  "pixel_stats")
			   ? 0
			   : -1;
}

// Per-pixel quantiles over time (pixel_quantile_kernels.hip).  Every argument is checked here; neither the values nor the state (the
// workspace of the one-call form) may overlap the frames or each other.
namespace
{
	bool pixel_quantiles_args(int w, int h, int npercents)
	{
		return w > 0 && h > 0 && (long long)w * h < (1ll << 31) && npercents >= 1 && npercents <= QUANTILE_MAX_PERCENTS;
	}
} // namespace

RIR_EXPORT int rir_pixel_quantiles_passes(void) { return PIXEL_QUANTILE_PASSES; }

RIR_EXPORT size_t rir_pixel_quantiles_state_bytes(int w, int h, int npercents)
{
	return pixel_quantiles_args(w, h, npercents) ? pixel_quantiles_state_bytes((int64_t)w * h, npercents) : 0;
}

RIR_EXPORT size_t rir_pixel_quantiles_workspace_bytes(int w, int h, int nframes, int npercents)
{
	return nframes >= 0 ? rir_pixel_quantiles_state_bytes(w, h, npercents) : 0;
}

RIR_EXPORT int rir_pixel_quantiles_push_device(const unsigned short *d_frames, int w, int h, int nframes, int npercents, int pass, void *d_state,
											   size_t state_bytes, void *stream)
{
	if (!device_ready())
		return -1;
	if (!pixel_quantiles_args(w, h, npercents) || nframes < 0 || pass < 0 || pass >= PIXEL_QUANTILE_PASSES)
		return refuse(__func__, "invalid argument (w, h >= 1 with w * h < 2^31, nframes >= 0, 1 <= npercents <= 8, "
								"0 <= pass < rir_pixel_quantiles_passes())");
	if (!d_frames || !d_state)
		return refuse(__func__, "null pointer");
	const size_t npx = (size_t)w * h, need = pixel_quantiles_state_bytes((int64_t)npx, npercents);
	if (!workspace_ok(__func__, d_state, state_bytes, need, "state", "rir_pixel_quantiles_state_bytes()"))
		return -1;
	if (nframes == 0)
		return 0;
	if (outputs_overlap({{d_frames, npx * nframes * 2}}, {{d_state, need}}))
		return refuse(__func__, "the state overlaps the frames");
	return hip_ok(launch_pixel_quantiles_count(d_frames, (int64_t)npx, nframes, npercents, pass, d_state, as_stream(stream)), "pixel_quantiles_push") ? 0
																																						: -1;
}

RIR_EXPORT int rir_pixel_quantiles_resolve_device(int w, int h, const float *percents, int npercents, int pass, long long total_frames, void *d_state,
												  size_t state_bytes, int *d_values, void *stream)
{
	if (!device_ready())
		return -1;
	if (!pixel_quantiles_args(w, h, npercents) || pass < 0 || pass >= PIXEL_QUANTILE_PASSES || total_frames < 0 || total_frames > 2147483647ll)
		return refuse(__func__, "invalid argument (w, h >= 1 with w * h < 2^31, 1 <= npercents <= 8, 0 <= pass < rir_pixel_quantiles_passes(), "
								"0 <= total_frames <= 2^31 - 1)");
	const bool last = pass == PIXEL_QUANTILE_PASSES - 1;
	if (!percents || !d_state || (last && !d_values))
		return refuse(__func__, "null pointer");
	QuantilePercents pc{};
	if (!percents_ok(__func__, percents, npercents, pc))
		return -1;
	const size_t npx = (size_t)w * h, need = pixel_quantiles_state_bytes((int64_t)npx, npercents);
	if (!workspace_ok(__func__, d_state, state_bytes, need, "state", "rir_pixel_quantiles_state_bytes()"))
		return -1;
	if (last && outputs_overlap({{d_state, need}}, {{d_values, npx * npercents * 4}}))
		return refuse(__func__, "the values overlap the state");
	return hip_ok(launch_pixel_quantiles_resolve((int64_t)npx, pc, npercents, pass, (uint32_t)total_frames, d_state, last ? d_values : nullptr,
												 as_stream(stream)),
				  "pixel_quantiles_resolve")
			   ? 0
			   : -1;
}

RIR_EXPORT int rir_pixel_quantiles_device(const unsigned short *d_frames, int w, int h, int nframes, const float *percents, int npercents,
										  int *d_values, void *d_work, size_t work_bytes, void *stream)
{
	if (!device_ready())
		return -1;
	if (!pixel_quantiles_args(w, h, npercents) || nframes < 0)
		return refuse(__func__, "invalid argument (w, h >= 1 with w * h < 2^31, nframes >= 0, 1 <= npercents <= 8)");
	if ((nframes > 0 && !d_frames) || !percents || !d_values || !d_work)
		return refuse(__func__, "null pointer");
	QuantilePercents pc{};
	if (!percents_ok(__func__, percents, npercents, pc))
		return -1;
	const size_t npx = (size_t)w * h, need = pixel_quantiles_state_bytes((int64_t)npx, npercents), out = npx * npercents * 4;
	if (!workspace_ok(__func__, d_work, work_bytes, need, "workspace", "rir_pixel_quantiles_workspace_bytes()"))
		return -1;
	if (outputs_overlap({{d_frames, npx * nframes * 2}}, {{d_values, out}, {d_work, need}})) // no frames: zero bytes, absent
		return refuse(__func__, "the values or the workspace overlap the frames or each other");
	hipStream_t st = as_stream(stream);
	if (nframes == 0) // no population: -1 everywhere
		return hip_ok(hipMemsetAsync(d_values, 0xFF, out, st), "hipMemsetAsync") ? 0 : -1;
	if (!hip_ok(hipMemsetAsync(d_work, 0, need, st), "hipMemsetAsync")) // the empty state
		return -1;
	for (int pass = 0; pass < PIXEL_QUANTILE_PASSES; ++pass)
		if (!hip_ok(launch_pixel_quantiles_count(d_frames, (int64_t)npx, nframes, npercents, pass, d_work, st), "pixel_quantiles") ||
			!hip_ok(launch_pixel_quantiles_resolve((int64_t)npx, pc, npercents, pass, (uint32_t)nframes, d_work,
												   pass == PIXEL_QUANTILE_PASSES - 1 ? d_values : nullptr, st),
					"pixel_quantiles"))
			return -1;
	return 0;
}

// Components tracked through time (track_kernels.hip).  Every argument is checked here; no output (workspace included) may overlap an
// input or another output, except d_dst == d_labels (relabelling in place).
RIR_EXPORT size_t rir_track_components_workspace_bytes(int w, int h, int nframes, int nlabels) { return track_workspace_bytes(w, h, nframes, nlabels); }

RIR_EXPORT int rir_track_components_device(const int *d_labels, const int *d_counts, int w, int h, int nframes, int nlabels, int *d_track_of, int *d_info,
										   int *d_first_frame, int *d_last_frame, int *d_first_label, int *d_components, int table_entries, int *d_dst,
										   void *d_work, size_t work_bytes, void *stream)
{
	if (!device_ready())
		return -1;
	if (!track_geometry_ok(w, h, nframes, nlabels) || table_entries < 1)
		return refuse(__func__, "invalid argument (w, h >= 1 with w * h <= 0x7FFF0000, nframes >= 0, nlabels >= 1 with "
								"nframes * nlabels <= 0x7FFF0000, table_entries >= 1)");
	if (!d_info || !d_first_frame || !d_last_frame || !d_first_label || !d_components || !d_work || (nframes > 0 && (!d_labels || !d_track_of)))
		return refuse(__func__, "null pointer");
	const size_t npx = (size_t)w * h, nodes = (size_t)nframes * nlabels, need = track_workspace_bytes(w, h, nframes, nlabels);
	if (!workspace_ok(__func__, d_work, work_bytes, need, "workspace", "rir_track_components_workspace_bytes()"))
		return -1;
	const size_t stack = npx * nframes * 4, table = (size_t)table_entries * 4;
	// d_dst == d_labels: the labels are left out of the inputs, their range is checked against everything else as the last output, d_dst
	if (outputs_overlap({{d_dst == d_labels ? nullptr : d_labels, stack}, {d_counts, (size_t)nframes * 4}},
						{{d_track_of, nodes * 4}, {d_info, 8}, {d_first_frame, table}, {d_last_frame, table}, {d_first_label, table},
						 {d_components, table}, {d_work, need}, {d_dst, stack}}))
		return refuse(__func__, "an output or the workspace overlaps an input or another output (only d_dst == d_labels may)");
	return hip_ok(launch_track_components(d_labels, d_counts, w, h, nframes, nlabels, d_track_of, d_info, d_first_frame, d_last_frame, d_first_label,
										  d_components, table_entries, d_dst, d_work, as_stream(stream)),
				  "track_components")
			   ? 0
			   : -1;
}

// Polygon label maps (polygon_kernels.hip).  Every argument is checked here; the maps and the workspace may not overlap an input or each other.
RIR_EXPORT size_t rir_polygon_map_workspace_bytes(int w, int h, int nmaps, int npoly, int max_pts)
{
	return polygon_map_workspace(w, h, nmaps, npoly, max_pts);
}

RIR_EXPORT int rir_polygon_map_device(const double *d_xy, const int *d_npts, const int *d_values, int npoly, int max_pts, int nmaps, int sets_per_map,
									  const double *d_shifts, int w, int h, int background, int *d_dst, void *d_work, size_t work_bytes, void *stream)
{
	if (!device_ready())
		return -1;
	if (!polygon_geometry_ok(w, h, nmaps, npoly, max_pts) || (sets_per_map != 0 && sets_per_map != 1))
		return refuse(__func__, "invalid argument (w, h >= 1 with w * h <= 0x7FFF0000, nmaps >= 0, 0 <= npoly <= 65536, 1 <= max_pts <= 1024, "
								"sets_per_map 0 or 1)");
	if (nmaps == 0)
		return 0;
	if (!d_dst || !d_work || (npoly > 0 && (!d_xy || !d_npts)))
		return refuse(__func__, "null pointer");
	const size_t need = polygon_map_workspace(w, h, nmaps, npoly, max_pts);
	if (!workspace_ok(__func__, d_work, work_bytes, need, "workspace", "rir_polygon_map_workspace_bytes()"))
		return -1;
	const size_t polys = (size_t)npoly * (sets_per_map ? nmaps : 1);
	if (outputs_overlap({{d_xy, polys * max_pts * 16}, {d_npts, polys * 4}, {d_values, (size_t)npoly * 4}, {d_shifts, (size_t)nmaps * 16}},
						{{d_dst, (size_t)w * h * nmaps * 4}, {d_work, need}}))
		return refuse(__func__, "the maps or the workspace overlap an input or each other");
	return hip_ok(launch_polygon_map(d_xy, d_npts, d_values, npoly, max_pts, nmaps, sets_per_map, d_shifts, w, h, background, d_dst, d_work,
									 as_stream(stream)),
				  "polygon_map")
			   ? 0
			   : -1;
}

// =====================================================================================================
// Reference entry points (host pointers, synchronous)
// =====================================================================================================

RIR_EXPORT int translate(int type, void *src, void *dst, int w, int h, float dx, float dy, void *background, const char *strategy)
{
	const int es = dtype_size(type);
	if (es == 0 || strategy_from_string(strategy) < 0) // signal_processing.cpp:40-41,70-71
		return -1;
	if (!device_ready())
		return -1;
	if (!src || !dst || !background || w <= 0 || h <= 0)
		return -1;
	HostScratch &s = scratch();
	std::lock_guard<std::mutex> g(s.mu);
	const size_t bytes = (size_t)w * h * es;
	hipStream_t st = default_stream();
	const bool keeps_dst = strategy_from_string(strategy) == TRANSLATE_UNCHANGED;
	const size_t off_at = (bytes + 63) & ~(size_t)63;
	if (!s.h_in.reserve(off_at + 64))
		return -1;
	// dst is an in/out buffer: "noborder" keeps whatever the caller put there (Filters.h:261-264), so only that
	// strategy needs the caller's dst where the kernel works; the others write every pixel
	float *off = reinterpret_cast<float *>(s.h_in.as<char>() + off_at); // (page-locked: the kernel reads the two floats from there)
	off[0] = dx, off[1] = dy;
	const void *in = stage_in(s, s.a, src, bytes, 0, st);
	void *out = in ? stage_out(s, s.b, dst, bytes, keeps_dst, st, in, bytes) : nullptr;
	if (!in || !out)
		return -1;
	if (rir_translate_device(type, in, out, w, h, 1, off, 0, background, strategy, st) != 0)
		return -1;
	return hand_out(s, dst, out, bytes, st) ? 0 : -1;
}

RIR_EXPORT int gaussian_filter(float *src, float *dst, int w, int h, float sigma)
{
	if (!device_ready())
		return -1;
	if (!src || !dst || w <= 0 || h <= 0)
		return -1;
	HostScratch &s = scratch();
	std::lock_guard<std::mutex> g(s.mu);
	const size_t bytes = (size_t)w * h * sizeof(float);
	hipStream_t st = default_stream();
	if (!s.h_in.reserve(bytes))
		return -1;
	const void *in = stage_in(s, s.a, src, bytes, 0, st);
	void *out = in ? stage_out(s, s.b, dst, bytes, false, st, in, bytes) : nullptr;
	if (!in || !out)
		return -1;
	if (rir_gaussian_filter_device(static_cast<const float *>(in), static_cast<float *>(out), w, h, 1, sigma, st) != 0)
		return -1;
	return hand_out(s, dst, out, bytes, st) ? 0 : -1;
}

// Extension: gaussian_filter of a uint16 image - what the reference's wrapper computes for one (it converts to float32 first,
// rir_signal_processing.py:85-113; every uint16 is a float32, so the conversion inside the kernel gives the same bits) - with half the bytes
// up the link.  Radius <= 4 (sigma < 2.5); -1 otherwise: the caller converts and takes gaussian_filter.
RIR_EXPORT int rir_gaussian_filter_u16(unsigned short *src, float *dst, int w, int h, float sigma)
{
	if (!device_ready())
		return -1;
	if (!src || !dst || w <= 0 || h <= 0 || !(sigma > 0) || gaussian_radius(sigma) > 4)
		return -1;
	HostScratch &s = scratch();
	std::lock_guard<std::mutex> g(s.mu);
	const size_t in_bytes = (size_t)w * h * 2, bytes = (size_t)w * h * sizeof(float);
	hipStream_t st = default_stream();
	if (!s.h_in.reserve(in_bytes))
		return -1;
	const void *in = stage_in(s, s.a, src, in_bytes, 0, st);
	void *out = in ? stage_out(s, s.b, dst, bytes, false, st, in, in_bytes) : nullptr;
	if (!in || !out)
		return -1;
	if (rir_gaussian_filter_u16_device(static_cast<const unsigned short *>(in), static_cast<float *>(out), w, h, 1, sigma, st) != 0)
		return -1;
	return hand_out(s, dst, out, bytes, st) ? 0 : -1;
}

static int find_median_host(unsigned short *pixels, unsigned char *mask, int size, float percent)
{
	if (!device_ready())
		return -1;
	if (!pixels || size <= 0)
		return 0;
	HostScratch &s = scratch();
	std::lock_guard<std::mutex> g(s.mu);
	hipStream_t st = default_stream();
	const size_t pbytes = (size_t)size * 2, mslot = (pbytes + 63) & ~(size_t)63;
	if (!s.b.reserve(65536 * sizeof(uint32_t)) || !s.c.reserve(sizeof(int)) || !s.h_in.reserve(mslot + (mask ? (size_t)size : 0)))
		return -1;
	const void *px = stage_in(s, s.a, pixels, pbytes, 0, st);
	const void *mk = mask ? stage_in(s, s.d, mask, (size_t)size, mslot, st) : nullptr;
	if (!px || (mask && !mk))
		return -1;
	if (rir_find_median_pixel_device(static_cast<const unsigned short *>(px), static_cast<const unsigned char *>(mk), size, 1, percent, s.c.as<int>(),
									 s.b.as<unsigned int>(), st) != 0)
		return -1;
	int res = 0;
	if (!hip_ok(hipMemcpyAsync(&res, s.c.ptr, sizeof(int), hipMemcpyDeviceToHost, st), "D2H") || !hip_ok(wait_stream(st), "sync"))
		return -1;
	return res;
}

RIR_EXPORT int find_median_pixel(unsigned short *pixels, int size, float percent) { return find_median_host(pixels, nullptr, size, percent); }
RIR_EXPORT int find_median_pixel_mask(unsigned short *pixels, unsigned char *mask, int size, float percent)
{
	return find_median_host(pixels, mask, size, percent);
}

// returns the object handle, 0 on error (signal_processing.h:77-80)
RIR_EXPORT int bad_pixels_create(unsigned short *first_image, int width, int height)
{
	if (!device_ready())
		return 0;
	if (!first_image || width <= 0 || height <= 0)
		return 0;
	HostScratch &s = scratch();
	std::lock_guard<std::mutex> g(s.mu);
	hipStream_t st = default_stream();
	const size_t bytes = (size_t)width * height * 2;
	// (the detector makes several passes over the image: it goes to device memory, whatever the switch says)
	if (!s.a.reserve(bytes) || !s.h_in.reserve(bytes))
		return 0;
	host_copy(s.h_in.ptr, first_image, bytes);
	if (!hip_ok(hipMemcpyAsync(s.a.ptr, s.h_in.ptr, bytes, hipMemcpyHostToDevice, st), "H2D"))
		return 0;
	return rir_bad_pixels_create_device(s.a.as<unsigned short>(), width, height, st);
}

RIR_EXPORT int bad_pixels_correct(int handle, unsigned short *in, unsigned short *out)
{
	auto bp = lookup_as<BadPixelsObject>(handle);
	if (!bp) // signal_processing.cpp:209-211
		return -1;
	if (!device_ready())
		return -1;
	if (!in || !out)
		return -1;
	HostScratch &s = scratch();
	std::lock_guard<std::mutex> g(s.mu);
	hipStream_t st = default_stream();
	const size_t bytes = (size_t)bp->width * bp->height * 2;
	if (!s.h_in.reserve(bytes))
		return -1;
	const void *src = stage_in(s, s.a, in, bytes, 0, st);
	void *dst = src ? stage_out(s, s.b, out, bytes, false, st, src, bytes) : nullptr;
	if (!src || !dst)
		return -1;
	if (rir_bad_pixels_correct_device(handle, static_cast<const unsigned short *>(src), static_cast<unsigned short *>(dst), 1, st) != 0)
		return -1;
	return hand_out(s, out, dst, bytes, st) ? 0 : -1;
}

// Extension: bad_pixels_correct -> gaussian_filter(sigma) -> translate(dx, dy, strategy) -> uint16 on ONE host image in one call (the reference's
// callers make the three calls, three trips over the link and two float images in between: configs[2] of BASELINE).  bad_pixels_handle 0: no
// repair.  Strategies "nearest" and "background"; the result is what rir_filter_chain_device gives (the three calls' result within one
// level, or exactly with rir_set_gaussian_reference_order(1)).  0 / -1.
RIR_EXPORT int rir_filter_chain(int bad_pixels_handle, unsigned short *in, unsigned short *out, int w, int h, float sigma, float dx, float dy,
								void *background, const char *strategy)
{
	if (!device_ready())
		return -1;
	if (!in || !out || w <= 0 || h <= 0)
		return -1;
	HostScratch &s = scratch();
	std::lock_guard<std::mutex> g(s.mu);
	hipStream_t st = default_stream();
	const size_t bytes = (size_t)w * h * 2;
	const size_t off_at = (bytes + 63) & ~(size_t)63;
	if (!s.h_in.reserve(off_at + 64))
		return -1;
	float *off = reinterpret_cast<float *>(s.h_in.as<char>() + off_at); // (page-locked: the kernel reads the two floats from there)
	off[0] = dx, off[1] = dy;
	const void *src = stage_in(s, s.a, in, bytes, 0, st);
	void *dst = src ? stage_out(s, s.b, out, bytes, false, st, src, bytes) : nullptr;
	if (!src || !dst)
		return -1;
	if (rir_filter_chain_device(bad_pixels_handle, static_cast<const unsigned short *>(src), static_cast<unsigned short *>(dst), w, h, 1, sigma, off, 0,
								background, strategy, st) != 0)
		return -1;
	return hand_out(s, out, dst, bytes, st) ? 0 : -1;
}

// ---- extension entries on host stacks: through the device in slabs, synchronous, 0 / -1 ---------------------------------------------------
namespace
{
	constexpr size_t HOST_SLAB_BYTES = (size_t)64 << 20; // what one slab of a host stack takes on the device at most, per kind of buffer

	struct Out // an output of a host stack entry: `cell` bytes per cell, at `dev` for the slab; a null `host`: not asked for
	{
		void *host;
		const void *dev;
		size_t cell;
	};

	// What a host stack entry queues on the library's stream.  A copy with a null address on either side is a group that was not asked for
	// (or an input that went up once): nothing is queued.  An entry with a failed step leaves through fail(), so that no copy is still on
	// its way into the caller's memory, or out of it, when the caller has the error.
	struct Stager
	{
		hipStream_t st = default_stream();

		// frames per slab: what HOST_SLAB_BYTES hold at each of the per-frame costs, at least one, at most nframes
		static int slab(int nframes, std::initializer_list<size_t> per_frame_bytes)
		{
			size_t n = (size_t)nframes;
			for (size_t b : per_frame_bytes)
				n = std::min(n, HOST_SLAB_BYTES / b);
			return (int)std::max<size_t>(1, n);
		}
		bool copy(void *dst, const void *src, size_t bytes, hipMemcpyKind kind) const
		{
			return !dst || !src || hip_ok(hipMemcpyAsync(dst, src, bytes, kind, st), "hipMemcpyAsync");
		}
		bool up(void *dev, const void *host, size_t bytes) const { return copy(dev, host, bytes, hipMemcpyHostToDevice); }
		bool down(void *host, const void *dev, size_t bytes) const { return copy(host, dev, bytes, hipMemcpyDeviceToHost); }
		// the slab's n cells of every output, to cell `at` of the caller's arrays
		template <size_t N>
		bool down(const Out (&outs)[N], size_t at, size_t n) const
		{
			for (const Out &o : outs)
				if (!down(o.host ? static_cast<char *>(o.host) + at * o.cell : nullptr, o.dev, n * o.cell))
					return false;
			return true;
		}
		bool wait(const char *what) const { return hip_ok(wait_stream(st), what); }
		int fail() const
		{
			(void)wait_stream(st); // what was queued is done before the buffers go
			return -1;
		}
	};
} // namespace

// The temporal median of a host stack, in slabs of output frames, each read with r frames of halo on either side (the windows of a slab's
// outputs are then those of the whole stack).
RIR_EXPORT int rir_temporal_median(const unsigned short *src, unsigned short *dst, int w, int h, int nframes, int window, int threshold, int rows)
{
	if (!device_ready())
		return -1;
	if (!src || !dst || w <= 0 || h <= 0 || nframes <= 0 || window < 1 || window > 63 || window % 2 == 0 || threshold < 0 || threshold > 65535 ||
		rows < 0 || rows > h)
		return refuse(__func__, "invalid argument (odd window 1..63, threshold 0..65535, 0 <= rows <= h)");
	const int r = window / 2;
	const size_t npx = (size_t)w * h, frame = npx * 2;
	const int slab = Stager::slab(nframes, {frame});
	DeviceBuffer in, out;
	if (!in.reserve(frame * (size_t)std::min(nframes, slab + 2 * r)) || !out.reserve(frame * slab))
		return -1;
	Stager s;
	for (int o = 0; o < nframes; o += slab)
	{
		const int count = std::min(slab, nframes - o), lo = std::max(0, o - r), hi = std::min(nframes, o + count + r);
		if (!s.up(in.ptr, src + lo * npx, frame * (hi - lo)) ||
			rir_temporal_median_device(in.as<unsigned short>(), out.as<unsigned short>(), w, h, hi - lo, o - lo, count, 1, window, threshold, rows, s.st) != 0 ||
			!s.down(dst + o * npx, out.ptr, frame * count) || !s.wait("temporal_median"))
			return s.fail();
	}
	return 0;
}

// The window filters of a host stack (frames are independent: any split gives the same bits; dst may be src): `bad` is what the entry's check
// found, filter(in, out, count, stream) its device entry over one slab.
namespace
{
	struct WindowOut // an output of a window filter on a host stack: `cell` bytes per pixel; a null `host`: not asked for
	{
		void *host;
		size_t cell;
	};

	// The walk: the stack goes up slab by slab - as many frames as HOST_SLAB_BYTES hold of the input and of the widest output -,
	// filter(in, d_outs, count, stream) runs the device entry over the slab (d_outs[k]: output k of the slab, null when not asked for),
	// and every output asked for comes down.
	template <size_t N, class Filter>
	int window_walk_host(const char *what, int type, const void *src, int w, int h, int nframes, const WindowOut (&outs)[N], Filter filter)
	{
		const size_t npx = (size_t)w * h, frame = npx * (type == 'H' ? 2 : 1);
		size_t widest = frame;
		for (const WindowOut &o : outs)
			widest = std::max(widest, o.host ? npx * o.cell : 0);
		const int slab = Stager::slab(nframes, {widest});
		DeviceBuffer in, dev[N];
		void *d_outs[N];
		if (!in.reserve(frame * slab))
			return -1;
		for (size_t k = 0; k < N; ++k)
		{
			d_outs[k] = outs[k].host ? dev[k].reserve(npx * outs[k].cell * slab) : nullptr;
			if (outs[k].host && !d_outs[k])
				return -1;
		}
		Stager s;
		for (int o = 0; o < nframes; o += slab)
		{
			const int count = std::min(slab, nframes - o);
			bool ok = s.up(in.ptr, static_cast<const char *>(src) + frame * o, frame * count) && filter(in.ptr, d_outs, count, s.st) == 0;
			for (size_t k = 0; ok && k < N; ++k)
				ok = s.down(outs[k].host ? static_cast<char *>(outs[k].host) + npx * outs[k].cell * o : nullptr, d_outs[k], npx * outs[k].cell * count);
			if (!ok || !s.wait(what))
				return s.fail();
		}
		return 0;
	}

	template <class Filter>
	int window_filter_host(const char *who, const char *what, const char *bad, int type, const void *src, void *dst, int w, int h, int nframes,
						   Filter filter)
	{
		bad = or_overlap(bad, type, src, dst, w, h, nframes, true);
		if (bad)
			return refuse(who, bad);
		if (nframes == 0)
			return 0;
		if (!device_ready())
			return -1;
		const WindowOut outs[] = {{dst, (size_t)(type == 'H' ? 2 : 1)}};
		return window_walk_host(what, type, src, w, h, nframes, outs,
								[&](const void *in, void *const *d_outs, int count, void *st) { return filter(in, d_outs[0], count, st); });
	}
} // namespace

RIR_EXPORT int rir_morphology(int type, const void *src, void *dst, int w, int h, int nframes, int op, int size_x, int size_y, int rows)
{
	return window_filter_host(__func__, "morphology", morphology_args(type, src, dst, w, h, nframes, op, size_x, size_y, rows), type, src, dst, w, h, nframes,
							  [=](const void *in, void *out, int count, void *st) {
								  return rir_morphology_device(type, in, out, w, h, count, op, size_x, size_y, rows, st);
							  });
}

RIR_EXPORT int rir_rank_filter(int type, const void *src, void *dst, int w, int h, int nframes, int rank, int size_x, int size_y, int rows)
{
	return window_filter_host(__func__, "rank_filter", rank_filter_args(type, src, dst, w, h, nframes, rank, size_x, size_y, rows), type, src, dst, w, h,
							  nframes, [=](const void *in, void *out, int count, void *st) {
								  return rir_rank_filter_device(type, in, out, w, h, count, rank, size_x, size_y, rows, st);
							  });
}

// The local window statistics of a host stack, through the window filters' walk with up to three outputs of their own cell sizes.
RIR_EXPORT int rir_local_stats(int type, const void *src, int w, int h, int nframes, int size_x, int size_y, int rows, int *sum, long long *sumsq, void *mean)
{
	if (const char *bad = local_stats_args(type, src, w, h, nframes, size_x, size_y, rows, sum, sumsq, mean))
		return refuse(__func__, bad);
	if (nframes == 0)
		return 0;
	if (!device_ready())
		return -1;
	const WindowOut outs[] = {{sum, 4}, {sumsq, 8}, {mean, (size_t)(type == 'H' ? 2 : 1)}};
	return window_walk_host("local_stats", type, src, w, h, nframes, outs, [=](const void *in, void *const *d, int count, void *st) {
		return rir_local_stats_device(type, in, w, h, count, size_x, size_y, rows, (int *)d[0], (long long *)d[1], d[2], st);
	});
}

RIR_EXPORT int rir_local_threshold(int type, const void *src, unsigned char *mask, int w, int h, int nframes, int size_x, int size_y, int rows, int k_num,
								   int k_den, int delta, int polarity)
{
	if (const char *bad = local_threshold_args(type, src, mask, w, h, nframes, size_x, size_y, rows, k_num, k_den, delta, polarity))
		return refuse(__func__, bad);
	if (nframes == 0)
		return 0;
	if (!device_ready())
		return -1;
	const WindowOut outs[] = {{mask, 1}};
	return window_walk_host("local_threshold", type, src, w, h, nframes, outs, [=](const void *in, void *const *d, int count, void *st) {
		return rir_local_threshold_device(type, in, (unsigned char *)d[0], w, h, count, size_x, size_y, rows, k_num, k_den, delta, polarity, st);
	});
}

// The distance transform of a host stack (frames are independent: any split gives the same bits); a slab is bounded by what a frame's input,
// outputs and workspace take on the device.  index may be null.
RIR_EXPORT int rir_distance_transform(int type, const void *src, int w, int h, int nframes, int background, int border, int rows, int *dist2, int *index)
{
	if (const char *bad = distance_transform_args(type, src, w, h, nframes, background, border, rows, dist2, index))
		return refuse(__func__, bad);
	if (nframes == 0)
		return 0;
	if (!device_ready())
		return -1;
	const size_t npx = (size_t)w * h, frame = npx * distance_cell_bytes(type), outs_bytes = npx * 4 * (index ? 2 : 1);
	const int slab = Stager::slab(nframes, {frame, outs_bytes, distance_frame_bytes(w, h)});
	const size_t work = distance_frame_bytes(w, h) * slab;
	DeviceBuffer in, o32, ws;
	if (!in.reserve(frame * slab) || !o32.reserve(outs_bytes * slab) || !ws.reserve(work))
		return -1;
	int *d_dist2 = o32.as<int>(), *d_index = index ? d_dist2 + npx * slab : nullptr;
	const Out outs[] = {{dist2, d_dist2, 4}, {index, d_index, 4}};
	Stager s;
	for (int o = 0; o < nframes; o += slab)
	{
		const int c = std::min(slab, nframes - o);
		if (!s.up(in.ptr, static_cast<const char *>(src) + frame * o, frame * c) ||
			rir_distance_transform_device(type, in.ptr, w, h, c, background, border, rows, d_dist2, d_index, ws.ptr, work, s.st) != 0 ||
			!s.down(outs, o * npx, c * npx) || !s.wait("distance_transform"))
			return s.fail();
	}
	return 0;
}

// Reconstruction of a host stack (frames are independent: any split gives the same bits): the mask, and the marker where there is one, go up
// slab by slab, the result comes down.
RIR_EXPORT int rir_reconstruct(int type, const void *mask, const void *marker, void *dst, int w, int h, int nframes, int method, int connectivity,
							   int marker_mode, int param, int output, int rows, int *rounds)
{
	if (const char *bad = reconstruct_args(type, mask, marker, dst, w, h, nframes, method, connectivity, marker_mode, param, output, rows))
		return refuse(__func__, bad);
	if (rounds)
		*rounds = 0;
	if (nframes == 0)
		return 0;
	if (!device_ready())
		return -1;
	const size_t frame = (size_t)w * h * (type == 'H' ? 2 : 1);
	const int slab = Stager::slab(nframes, {frame});
	const size_t work = RECONSTRUCT_FRAME_BYTES * slab;
	DeviceBuffer in, seed, out, ws;
	if (!in.reserve(frame * slab) || (marker && !seed.reserve(frame * slab)) || !out.reserve(frame * slab) || !ws.reserve(work))
		return -1;
	Stager s;
	for (int o = 0; o < nframes; o += slab)
	{
		const int c = std::min(slab, nframes - o);
		int took = 0;
		if (!s.up(in.ptr, static_cast<const char *>(mask) + frame * o, frame * c) ||
			!s.up(marker ? seed.ptr : nullptr, marker ? static_cast<const char *>(marker) + frame * o : nullptr, frame * c) ||
			rir_reconstruct_device(type, in.ptr, marker ? seed.ptr : nullptr, out.ptr, w, h, c, method, connectivity, marker_mode, param, output, rows, ws.ptr,
								   work, &took, s.st) != 0 ||
			!s.down(static_cast<char *>(dst) + frame * o, out.ptr, frame * c) || !s.wait("reconstruct"))
			return s.fail();
		if (rounds)
			*rounds = std::max(*rounds, took);
	}
	return 0;
}

// Per-region statistics of a host stack: a shared label map goes up once, per-frame maps go up with their frames; a slab is also bounded by
// what its outputs and workspace take on the device.
RIR_EXPORT int rir_region_stats(const unsigned short *frames, const int *labels, int w, int h, int nframes, int labels_per_frame, int nregions,
								int *count, long long *sum, long long *sumsq, int *min, int *max, int *argmin, int *argmax)
{
	if (!device_ready())
		return -1;
	if (!region_stats_args(w, h, nframes, labels_per_frame, nregions) || !frames || !labels || !count || !sum || !sumsq || !min || !max || !argmin ||
		!argmax)
		return refuse(__func__, "invalid argument (w, h >= 1 with w * h < 2^31, nframes >= 0, labels_per_frame 0 or 1, 1 <= nregions <= 2^24, "
								"no null pointer)");
	if (nframes == 0)
		return 0;
	const size_t npx = (size_t)w * h, K = (size_t)nregions;
	const int slab = Stager::slab(nframes, {npx * 2, K * (5 * 4 + 2 * 8 + 32)}); // a frame; its outputs and workspace
	const size_t cells = (size_t)slab * K, work = region_stats_workspace((int64_t)npx, slab, nregions);
	DeviceBuffer fr, lab, o32, o64, ws;
	if (!fr.reserve(npx * 2 * slab) || !lab.reserve(npx * 4 * (labels_per_frame ? slab : 1)) || !o32.reserve(cells * 4 * 5) || !o64.reserve(cells * 8 * 2) ||
		!ws.reserve(work))
		return -1;
	int *d32 = o32.as<int>();
	long long *d64 = o64.as<long long>();
	const Out outs[] = {{count, d32, 4}, {min, d32 + cells, 4}, {max, d32 + 2 * cells, 4}, {argmin, d32 + 3 * cells, 4}, {argmax, d32 + 4 * cells, 4},
						{sum, d64, 8}, {sumsq, d64 + cells, 8}};
	Stager s;
	if (!s.up(lab.ptr, labels_per_frame ? nullptr : labels, npx * 4))
		return s.fail();
	for (int o = 0; o < nframes; o += slab)
	{
		const int c = std::min(slab, nframes - o);
		if (!s.up(fr.ptr, frames + o * npx, npx * 2 * c) || !s.up(lab.ptr, labels_per_frame ? labels + o * npx : nullptr, npx * 4 * c) ||
			rir_region_stats_device(fr.as<unsigned short>(), lab.as<int>(), w, h, c, labels_per_frame, nregions, d32, d64, d64 + cells, d32 + cells,
									d32 + 2 * cells, d32 + 3 * cells, d32 + 4 * cells, ws.ptr, work, s.st) != 0 ||
			!s.down(outs, o * K, c * K) || !s.wait("region_stats"))
			return s.fail();
	}
	return 0;
}

// Per-region geometry of host label maps, weighted by a host stack when `frames` is given; staged as rir_region_stats stages its arguments
// (without frames the slabs are label maps).
RIR_EXPORT int rir_region_geometry(const int *labels, const unsigned short *frames, int w, int h, int nframes, int labels_per_frame, int nregions,
								   int *count, int *bbox, long long *moments, long long *weighted)
{
	if (!device_ready())
		return -1;
	if (!region_geometry_args(w, h, nframes, labels_per_frame, nregions, frames != nullptr) || !labels || !count || !bbox || !moments ||
		(frames != nullptr) != (weighted != nullptr))
		return refuse(__func__, std::string(REGION_GEOMETRY_ARGS) + ", or a null pointer (weighted is null exactly when frames is)");
	if (nframes == 0)
		return 0;
	const size_t npx = (size_t)w * h, frame = npx * (frames ? 2 : 0) + npx * (labels_per_frame ? 4 : 0), K = (size_t)nregions;
	const int slab = Stager::slab(nframes, {std::max<size_t>(frame, 1), K * (4 + 16 + 40 + 24)}); // what goes up per frame; a frame's outputs
	const size_t cells = (size_t)slab * K;
	DeviceBuffer fr, lab, o32, o64, ws;
	if ((frames && !fr.reserve(npx * 2 * slab)) || !lab.reserve(npx * 4 * (labels_per_frame ? slab : 1)) || !o32.reserve(cells * 4 * 5) ||
		!o64.reserve(cells * 8 * 8) || !ws.reserve(GEOMETRY_WORK_BYTES))
		return -1;
	int *d_count = o32.as<int>(), *d_bbox = d_count + cells;
	long long *d_mom = o64.as<long long>(), *d_wgt = frames ? d_mom + 5 * cells : nullptr;
	const Out outs[] = {{count, d_count, 4}, {bbox, d_bbox, 16}, {moments, d_mom, 40}, {weighted, d_wgt, 24}};
	Stager s;
	if (!s.up(lab.ptr, labels_per_frame ? nullptr : labels, npx * 4))
		return s.fail();
	for (int o = 0; o < nframes; o += slab)
	{
		const int c = std::min(slab, nframes - o);
		if (!s.up(fr.ptr, frames ? frames + o * npx : nullptr, npx * 2 * c) || !s.up(lab.ptr, labels_per_frame ? labels + o * npx : nullptr, npx * 4 * c) ||
			rir_region_geometry_device(lab.as<int>(), frames ? fr.as<unsigned short>() : nullptr, w, h, c, labels_per_frame, nregions, d_count, d_bbox, d_mom,
									   d_wgt, ws.ptr, GEOMETRY_WORK_BYTES, s.st) != 0 ||
			!s.down(outs, o * K, c * K) || !s.wait("region_geometry"))
			return s.fail();
	}
	return 0;
}

// Per-region quantiles of a host stack, staged as rir_region_stats stages its arguments.
RIR_EXPORT int rir_region_quantiles(const unsigned short *frames, const int *labels, int w, int h, int nframes, int labels_per_frame, int nregions,
									const float *percents, int npercents, int *count, int *values)
{
	if (!device_ready())
		return -1;
	if (!region_quantiles_args(w, h, nframes, labels_per_frame, nregions, npercents) || !frames || !labels || !percents || !count || !values)
		return refuse(__func__, "invalid argument (w, h >= 1 with w * h < 2^31, nframes >= 0, labels_per_frame 0 or 1, 1 <= nregions <= 65536, "
								"1 <= npercents <= 8, no null pointer)");
	QuantilePercents pc{};
	if (!percents_ok(__func__, percents, npercents, pc))
		return -1;
	if (nframes == 0)
		return 0;
	const size_t npx = (size_t)w * h, K = (size_t)nregions, Q = (size_t)npercents;
	const int slab = Stager::slab(nframes, {npx * 2, K * 4 * (1 + Q) + region_quantiles_frame_bytes(nregions, npercents)}); // as rir_region_stats
	const size_t cells = (size_t)slab * K, work = rir_region_quantiles_workspace_bytes(w, h, slab, labels_per_frame, nregions, npercents);
	DeviceBuffer fr, lab, o32, ws;
	if (!fr.reserve(npx * 2 * slab) || !lab.reserve(npx * 4 * (labels_per_frame ? slab : 1)) || !o32.reserve(cells * 4 * (1 + Q)) || !ws.reserve(work))
		return -1;
	int *d_count = o32.as<int>(), *d_values = d_count + cells;
	const Out outs[] = {{count, d_count, 4}, {values, d_values, Q * 4}};
	Stager s;
	if (!s.up(lab.ptr, labels_per_frame ? nullptr : labels, npx * 4))
		return s.fail();
	for (int o = 0; o < nframes; o += slab)
	{
		const int c = std::min(slab, nframes - o);
		if (!s.up(fr.ptr, frames + o * npx, npx * 2 * c) || !s.up(lab.ptr, labels_per_frame ? labels + o * npx : nullptr, npx * 4 * c) ||
			rir_region_quantiles_device(fr.as<unsigned short>(), lab.as<int>(), w, h, c, labels_per_frame, nregions, percents, npercents, d_count, d_values,
										ws.ptr, work, s.st) != 0 ||
			!s.down(outs, o * K, c * K) || !s.wait("region_quantiles"))
			return s.fail();
	}
	return 0;
}

// Per-region histograms of a host stack, staged as rir_region_stats stages its arguments; without labels no map goes up.  count and
// outside may be null.
RIR_EXPORT int rir_region_histogram(const unsigned short *frames, const int *labels, int w, int h, int rows, int nframes, int labels_per_frame,
									int nregions, int lo, int width, int nbins, int *count, int *hist, int *outside)
{
	if (!region_histogram_args(labels != nullptr, w, h, rows, nframes, labels_per_frame, nregions, lo, width, nbins))
		return refuse(__func__, REGION_HISTOGRAM_ARGS);
	if (!frames || !hist)
		return refuse(__func__, "null pointer (only labels, count and outside may be null)");
	if (nframes == 0)
		return 0;
	if (!device_ready())
		return -1;
	const size_t npx = (size_t)w * h, K = (size_t)nregions, B = (size_t)nbins;
	const int slab = Stager::slab(nframes, {npx * 2, K * (B + 3) * 4}); // a frame; its outputs
	const size_t cells = (size_t)slab * K;
	DeviceBuffer fr, lab, o32, ws;
	if (!fr.reserve(npx * 2 * slab) || (labels && !lab.reserve(npx * 4 * (labels_per_frame ? slab : 1))) || !o32.reserve(cells * (B + 3) * 4) ||
		!ws.reserve(HISTOGRAM_WORK_BYTES))
		return -1;
	int *d_hist = o32.as<int>(), *d_outside = d_hist + cells * B, *d_count = d_outside + cells * 2;
	const Out outs[] = {{count, d_count, 4}, {hist, d_hist, B * 4}, {outside, d_outside, 8}};
	Stager s;
	if (!s.up(lab.ptr, labels_per_frame ? nullptr : labels, npx * 4))
		return s.fail();
	for (int o = 0; o < nframes; o += slab)
	{
		const int c = std::min(slab, nframes - o);
		if (!s.up(fr.ptr, frames + o * npx, npx * 2 * c) || !s.up(lab.ptr, labels_per_frame ? labels + o * npx : nullptr, npx * 4 * c) ||
			rir_region_histogram_device(fr.as<unsigned short>(), labels ? lab.as<int>() : nullptr, w, h, rows, c, labels_per_frame, nregions, lo, width, nbins,
										d_count, d_hist, d_outside, ws.ptr, HISTOGRAM_WORK_BYTES, s.st) != 0 ||
			!s.down(outs, o * K, c * K) || !s.wait("region_histogram"))
			return s.fail();
	}
	return 0;
}

// Per-pixel statistics over time of a host stack: the slabs accumulate on the device, the outputs come back once.  A group (sum, sumsq /
// min, max, argmin, argmax) may be null.
RIR_EXPORT int rir_pixel_stats(const unsigned short *frames, int w, int h, int nframes, long long *sum, long long *sumsq, int *min, int *max,
							   int *argmin, int *argmax)
{
	if (!device_ready())
		return -1;
	const bool sums = sum || sumsq, extremes = min || max || argmin || argmax;
	if (!pixel_stats_args(w, h, nframes) || !frames || (sums && (!sum || !sumsq)) || (extremes && (!min || !max || !argmin || !argmax)) ||
		(!sums && !extremes))
		return refuse(__func__, "invalid argument (w, h >= 1 with w * h < 2^31, nframes >= 0, frames given, each group of outputs all given "
								"or all null and one given)");
	if (nframes == 0)
		return 0;
	const size_t npx = (size_t)w * h;
	const int slab = Stager::slab(nframes, {npx * 2});
	const size_t work = pixel_stats_workspace((int64_t)npx, slab);
	DeviceBuffer fr, o32, o64, ws;
	if (!fr.reserve(npx * 2 * slab) || !ws.reserve(work) || (sums && !o64.reserve(npx * 8 * 2)) || (extremes && !o32.reserve(npx * 4 * 4)))
		return -1;
	const auto d64 = [&](int k) { return sums ? o64.as<long long>() + k * npx : nullptr; }; // a group not asked for stays null
	const auto d32 = [&](int k) { return extremes ? o32.as<int>() + k * npx : nullptr; };
	const Out outs[] = {{sum, d64(0), 8}, {sumsq, d64(1), 8}, {min, d32(0), 4}, {max, d32(1), 4}, {argmin, d32(2), 4}, {argmax, d32(3), 4}};
	Stager s;
	for (int o = 0; o < nframes; o += slab)
	{
		const int c = std::min(slab, nframes - o);
		if (!s.up(fr.ptr, frames + o * npx, npx * 2 * c) ||
			rir_pixel_stats_device(fr.as<unsigned short>(), w, h, c, o, o != 0, d64(0), d64(1), d32(0), d32(1), d32(2), d32(3), ws.ptr, work, s.st) != 0)
			return s.fail();
	}
	return s.down(outs, 0, npx) && s.wait("pixel_stats") ? 0 : s.fail();
}

// Per-pixel quantiles over time of a host stack.  A stack of at most PIXEL_QUANTILES_RESIDENT_BYTES goes up once and runs the one-call form; a
// larger one goes up in slabs, once per pass, through the streaming form: the same bits.
constexpr size_t PIXEL_QUANTILES_RESIDENT_BYTES = (size_t)256 << 20;

RIR_EXPORT int rir_pixel_quantiles(const unsigned short *frames, int w, int h, int nframes, const float *percents, int npercents, int *values)
{
	if (!device_ready())
		return -1;
	if (!pixel_quantiles_args(w, h, npercents) || nframes < 0 || (nframes > 0 && !frames) || !percents || !values)
		return refuse(__func__, "invalid argument (w, h >= 1 with w * h < 2^31, nframes >= 0, 1 <= npercents <= 8, no null pointer)");
	QuantilePercents pc{};
	if (!percents_ok(__func__, percents, npercents, pc))
		return -1;
	const size_t npx = (size_t)w * h, frame = npx * 2, out = npx * npercents * 4, state = pixel_quantiles_state_bytes((int64_t)npx, npercents);
	const bool resident = frame * (size_t)nframes <= PIXEL_QUANTILES_RESIDENT_BYTES;
	const int slab = resident ? nframes : Stager::slab(nframes, {frame});
	DeviceBuffer fr, o32, ws;
	if ((nframes > 0 && !fr.reserve(frame * slab)) || !o32.reserve(out) || !ws.reserve(state))
		return -1;
	Stager s;
	bool ok;
	if (resident) // (no frames: nothing goes up, and the one-call form writes -1 everywhere)
		ok = s.up(fr.ptr, frames, frame * nframes) &&
			 rir_pixel_quantiles_device(fr.as<unsigned short>(), w, h, nframes, percents, npercents, o32.as<int>(), ws.ptr, state, s.st) == 0;
	else
	{
		ok = hip_ok(hipMemsetAsync(ws.ptr, 0, state, s.st), "hipMemsetAsync");
		for (int pass = 0; ok && pass < PIXEL_QUANTILE_PASSES; ++pass)
		{
			for (int o = 0; ok && o < nframes; o += slab)
			{
				const int c = std::min(slab, nframes - o);
				// the copy waits for the kernels that read the slab before it: one stream
				ok = s.up(fr.ptr, frames + o * npx, frame * c) &&
					 rir_pixel_quantiles_push_device(fr.as<unsigned short>(), w, h, c, npercents, pass, ws.ptr, state, s.st) == 0;
			}
			ok = ok && rir_pixel_quantiles_resolve_device(w, h, percents, npercents, pass, nframes, ws.ptr, state, o32.as<int>(), s.st) == 0;
		}
	}
	return ok && s.down(values, o32.ptr, out) && s.wait("pixel_quantiles") ? 0 : s.fail();
}

// Polygon label maps into host memory.  The polygons, values and shifts go up once; the maps are made on the device slab by slab, each slab
// from its own sets and shifts, and come back slab by slab.
RIR_EXPORT int rir_polygon_map(const double *xy, const int *npts, const int *values, int npoly, int max_pts, int nmaps, int sets_per_map,
							   const double *shifts, int w, int h, int background, int *dst)
{
	if (!device_ready())
		return -1;
	if (!polygon_geometry_ok(w, h, nmaps, npoly, max_pts) || (sets_per_map != 0 && sets_per_map != 1) || (nmaps > 0 && !dst) ||
		(nmaps > 0 && npoly > 0 && (!xy || !npts)))
		return refuse(__func__, "invalid argument (w, h >= 1 with w * h <= 0x7FFF0000, nmaps >= 0, 0 <= npoly <= 65536, 1 <= max_pts <= 1024, "
								"sets_per_map 0 or 1, no null pointer)");
	if (nmaps == 0)
		return 0;
	const size_t npx = (size_t)w * h, polys = (size_t)npoly * (sets_per_map ? nmaps : 1), set_doubles = (size_t)npoly * max_pts * 2;
	const int slab = Stager::slab(nmaps, {npx * 4});
	const size_t work = polygon_map_workspace(w, h, slab, npoly, max_pts);
	DeviceBuffer dxy, dn, dv, ds, maps, ws; // those of inputs that are not given stay null
	if (!maps.reserve(npx * 4 * slab) || !ws.reserve(work) || (npoly > 0 && (!dxy.reserve(polys * max_pts * 16) || !dn.reserve(polys * 4))) ||
		(npoly > 0 && values && !dv.reserve((size_t)npoly * 4)) || (shifts && !ds.reserve((size_t)nmaps * 16)))
		return -1;
	Stager s;
	if (!s.up(dxy.ptr, xy, polys * max_pts * 16) || !s.up(dn.ptr, npts, polys * 4) || !s.up(dv.ptr, values, (size_t)npoly * 4) ||
		!s.up(ds.ptr, shifts, (size_t)nmaps * 16))
		return s.fail();
	for (int o = 0; o < nmaps; o += slab)
	{
		const int c = std::min(slab, nmaps - o);
		const size_t set = sets_per_map ? (size_t)o : 0;
		if (rir_polygon_map_device(dxy.ptr ? dxy.as<double>() + set * set_doubles : nullptr, dn.ptr ? dn.as<int>() + set * npoly : nullptr, dv.as<int>(),
								   npoly, max_pts, c, sets_per_map, ds.ptr ? ds.as<double>() + (size_t)o * 2 : nullptr, w, h, background, maps.as<int>(),
								   ws.ptr, work, s.st) != 0 ||
			!s.down(dst + o * npx, maps.ptr, npx * 4 * c) || !s.wait("polygon_map"))
			return s.fail();
	}
	return 0;
}

RIR_EXPORT void bad_pixels_destroy(int handle)
{
	if (lookup_as<BadPixelsObject>(handle))
		remove_object(handle);
}

// hash_bytes (signal_processing.cpp:337-392): 64-bit multiply/xor-shift hash used by the Python
// cache helpers.  Host-side utility, restated here so the symbol exists in the drop-in library.
RIR_EXPORT size_t hash_bytes(void *_ptr, size_t len)
{
	const uint64_t m = 14313749767032793493ULL, seed = 3782874213ULL, r = 47ULL;
	const unsigned char *ptr = static_cast<const unsigned char *>(_ptr);
	uint64_t h = seed ^ (len * m);
	const size_t nblocks = len / 8;
	for (size_t i = 0; i < nblocks; ++i, ptr += 8)
	{
		uint64_t k;
		std::memcpy(&k, ptr, 8);
		k *= m;
		k ^= k >> r;
		k *= m;
		h ^= k;
		h *= m;
	}
	const size_t tail = len & 7U;
	if (tail)
	{
		for (size_t i = tail; i-- > 0;)
			h ^= (uint64_t)ptr[i] << (8 * i);
		h *= m;
	}
	h ^= h >> r;
	h *= m;
	h ^= h >> r;
	return (size_t)h;
}

// ---- connected components (label_kernels.hip) -----------------------------------------------------------------------------------
namespace
{
	int cell_bytes_of(int type)
	{ // what `==` means for the reference's cell types (signal_processing.cpp:228-263): integers by their bits, floating point as IEEE
		switch (type)
		{
		case 'f':
			return -4;
		case 'd':
			return -8;
		default:
			return dtype_size(type); // 0: unknown
		}
	}
	// `(U)background` with U = int (Filters.h:535): the host's own conversion of the cell type, at run time like the reference's
	int background_as_int(int type, const void *bg)
	{
		switch (type)
		{
		case '?':
		case 'B':
			return (int)*static_cast<const unsigned char *>(bg);
		case 'b':
			return (int)*static_cast<const signed char *>(bg);
		case 'h':
			return (int)*static_cast<const short *>(bg);
		case 'H':
			return (int)*static_cast<const unsigned short *>(bg);
		case 'i':
			return *static_cast<const int *>(bg);
		case 'I':
			return (int)*static_cast<const unsigned int *>(bg);
		case 'l':
			return (int)*static_cast<const long long *>(bg);
		case 'L':
			return (int)*static_cast<const unsigned long long *>(bg);
		case 'f':
		{
			volatile float f = *static_cast<const float *>(bg);
			return (int)f;
		}
		case 'd':
		{
			volatile double d = *static_cast<const double *>(bg);
			return (int)d;
		}
		default:
			return 0;
		}
	}
} // namespace

RIR_EXPORT size_t rir_label_workspace_bytes(int w, int h) { return label_workspace_bytes(w, h, 1); }
RIR_EXPORT size_t rir_label_workspace_bytes_batch(int w, int h, int nframes) { return label_workspace_bytes(w, h, nframes); }

// A batch of images [nframes][h][w] in device memory, every one labelled on its own (five launches for the whole batch).
RIR_EXPORT int rir_label_images_device(int type, const void *d_src, int *d_dst, int w, int h, int nframes, const void *background, double *d_xy,
									   int *d_area, int table_entries, int *d_count, void *d_work, size_t work_bytes, void *stream)
{
	const int cell = cell_bytes_of(type);
	if (cell == 0)
		return -1;
	if (!device_ready())
		return -1;
	const size_t need = label_workspace_bytes(w, h, nframes);
	if (need == 0 || work_bytes < need || ((uintptr_t)d_work & 7) || table_entries < 1)
		return -1;
	return hip_ok(launch_label_images(cell, d_src, background, w, h, nframes, d_dst, d_xy, d_area, table_entries, d_count, d_work, as_stream(stream)),
				  "label_image")
			   ? 0
			   : -1;
}
RIR_EXPORT int rir_label_image_device(int type, const void *d_src, int *d_dst, int w, int h, const void *background, double *d_xy, int *d_area,
									  int *d_count, void *d_work, size_t work_bytes, void *stream)
{
	if (w <= 0 || h <= 0 || (int64_t)w * h >= 0x7FFFFFFFLL)
		return -1;
	return rir_label_images_device(type, d_src, d_dst, w, h, 1, background, d_xy, d_area, w * h + 1, d_count, d_work, work_bytes, stream);
}

// Hot spots labelled straight from uint16 frames (label_kernels.hip).  Refusals as rir_label_images_device's: -1.
RIR_EXPORT size_t rir_label_hot_spots_workspace_bytes(int w, int h, int nframes) { return label_hot_spots_workspace_bytes(w, h, nframes); }

RIR_EXPORT int rir_label_hot_spots_device(const unsigned short *d_frames, int w, int h, int nframes, int rows, int low, const int *d_low_map, int use_high,
										  int high, const int *d_high_map, int min_area, int max_area, int clear_border, int *d_dst, int *d_first,
										  int *d_area, int table_entries, int *d_count, void *d_work, size_t work_bytes, void *stream)
{
	if (!device_ready())
		return -1;
	const size_t need = label_hot_spots_workspace_bytes(w, h, nframes);
	if (need == 0 || rows < 1 || rows > h || min_area < 1 || max_area < min_area || table_entries < 1)
		return refuse(__func__, "invalid argument (w, h >= 1 with w * h <= 0x7FFF0000, 1 <= nframes <= 65535, 1 <= rows <= h, "
								"1 <= min_area <= max_area, table_entries >= 1)");
	if (!d_frames || !d_dst || !d_first || !d_area || !d_count || !d_work)
		return refuse(__func__, "null pointer");
	if (!workspace_ok(__func__, d_work, work_bytes, need, "workspace", "rir_label_hot_spots_workspace_bytes()"))
		return -1;
	const size_t npx = (size_t)w * h, table = (size_t)nframes * table_entries * 4;
	if (outputs_overlap({{d_frames, npx * nframes * 2}, {d_low_map, npx * 4}, {use_high ? d_high_map : nullptr, npx * 4}},
						{{d_dst, npx * nframes * 4}, {d_first, table}, {d_area, table}, {d_count, (size_t)nframes * 4}, {d_work, need}}))
		return refuse(__func__, "an output or the workspace overlaps an input or another output");
	return hip_ok(launch_label_hot_spots(d_frames, w, h, nframes, rows, low, d_low_map, use_high != 0, high, d_high_map, min_area, max_area,
										 clear_border != 0, d_dst, d_first, d_area, table_entries, d_count, d_work, as_stream(stream)),
				  "label_hot_spots")
			   ? 0
			   : -1;
}

RIR_EXPORT int rir_keep_largest_areas_device(int type, const void *d_src, int *d_dst, int w, int h, int nframes, const void *background, int foreground,
											 void *d_work, size_t work_bytes, void *stream)
{
	const int cell = cell_bytes_of(type);
	if (cell == 0 || !background)
		return -1;
	if (!device_ready())
		return -1;
	const size_t need = label_workspace_bytes(w, h, nframes);
	if (need == 0 || work_bytes < need || ((uintptr_t)d_work & 7))
		return -1;
	return hip_ok(launch_keep_largest_areas(cell, d_src, background, w, h, nframes, d_dst, foreground, background_as_int(type, background), d_work,
											as_stream(stream)),
				  "keep_largest_area")
			   ? 0
			   : -1;
}
RIR_EXPORT int rir_keep_largest_area_device(int type, const void *d_src, int *d_dst, int w, int h, const void *background, int foreground,
											void *d_work, size_t work_bytes, void *stream)
{
	return rir_keep_largest_areas_device(type, d_src, d_dst, w, h, 1, background, foreground, d_work, work_bytes, stream);
}

// The image goes to device memory (the passes read it several times); the labels come back through the page-locked staging buffer
// like every other image of this file, the small tables (one entry per component) are written over the link by the kernel itself.
static int label_host(int type, void *src, int *dst, int w, int h, void *background, double *out_xy, int *out_area, bool keep, int foreground)
{
	const int es = dtype_size(type);
	if (es == 0) // signal_processing.cpp:261-262, :313-314
		return -1;
	if (!device_ready())
		return -1;
	if (!src || !dst || !background || w < 0 || h < 0 || (!keep && (!out_xy || !out_area)))
		return -1;
	if (w == 0 || h == 0)
	{ // no pixel: the table holds the background's entry alone (Filters.h:489, Label() = (-1, -1), area 0)
		if (keep)
			return 0;
		out_xy[0] = out_xy[1] = -1.0;
		out_area[0] = 0;
		return 1;
	}
	const size_t work = label_workspace_bytes(w, h, 1);
	if (work == 0)
	{
		log_error("label_image: image too large");
		return -1;
	}
	HostScratch &s = scratch();
	std::lock_guard<std::mutex> g(s.mu);
	hipStream_t st = default_stream();
	const size_t n = (size_t)w * h, in_bytes = n * es, out_bytes = n * sizeof(int);
	const size_t xy_bytes = (n + 1) * 2 * sizeof(double), area_bytes = (n + 1) * sizeof(int);
	if (!s.h_in.reserve(in_bytes) || !s.a.reserve(in_bytes) || !s.c.reserve(work) || (!keep && !s.h_tab.reserve(xy_bytes + area_bytes + 64)))
		return -1;
	host_copy(s.h_in.ptr, src, in_bytes);
	if (!hip_ok(hipMemcpyAsync(s.a.ptr, s.h_in.ptr, in_bytes, hipMemcpyHostToDevice, st), "H2D"))
		return -1;
	void *out = stage_out(s, s.b, dst, out_bytes, false, st);
	if (!out)
		return -1;
	if (keep)
	{
		if (rir_keep_largest_area_device(type, s.a.ptr, static_cast<int *>(out), w, h, background, foreground, s.c.ptr, s.c.cap, st) != 0)
			return -1;
		return hand_out(s, dst, out, out_bytes, st) ? 0 : -1;
	}
	double *xy = s.h_tab.as<double>();
	int *area = reinterpret_cast<int *>(s.h_tab.as<char>() + xy_bytes);
	int *count = reinterpret_cast<int *>(s.h_tab.as<char>() + xy_bytes + area_bytes);
	*count = -1;
	if (rir_label_image_device(type, s.a.ptr, static_cast<int *>(out), w, h, background, xy, area, count, s.c.ptr, s.c.cap, st) != 0)
		return -1;
	if (!hand_out(s, dst, out, out_bytes, st)) // (waits for the stream: the tables are complete)
		return -1;
	const int labels = *count;
	if (labels < 1 || (size_t)labels > n + 1)
		return -1;
	std::memcpy(out_xy, xy, (size_t)labels * 2 * sizeof(double));
	std::memcpy(out_area, area, (size_t)labels * sizeof(int));
	return labels;
}

// reference signal_processing.cpp:224-266: the number of table entries (components + 1), -1 on an unknown type.  out_xy / out_area
// receive that many entries (the caller sizes them; one entry per pixel plus one is always enough).
RIR_EXPORT int label_image(int type, void *src, int *dst, int w, int h, void *background, double *out_xy, int *out_area)
{
	return label_host(type, src, dst, w, h, background, out_xy, out_area, false, 0);
}
// reference signal_processing.cpp:276-318: 0, -1 on an unknown type
RIR_EXPORT int keep_largest_area(int type, void *src, int *dst, int w, int h, void *background, int foreground)
{
	return label_host(type, src, dst, w, h, background, nullptr, nullptr, true, foreground);
}
