// Adaptive temporal downsampling with max-hold: the reference's VideoDownsampler (src/cpp/video_io/h264.cpp:117-451, h264.h:13-30) on
// frames that lie in device memory.  Out of a sequence about one image in `factor` is kept, more while the scene changes, and every kept
// image is the per-pixel maximum of the images since the last kept one.  The contract is restated with rir_downsampler_push_device in
// include/rir_amd_device.h; this unit holds the scalar keep / drop recurrence (a pure host function, rir_downsample_decide) and the stream
// object that runs the two device passes of downsample_kernels.hip around it.
//
// Deviations from the reference, all documented in the header and DESIGN.md section 7:
//   - the sums of |d| and d^2 are exact int64 (the reference accumulates in double - the same value while size * 65535^2 < 2^53 - and squares
//     in int, undefined for d > 46340); size > 2^31 - 1 is refused;
//   - a negative radicand of the statistic, which only the rounding of x * x can produce, gives 0 and not NaN (the reference would hand a
//     NaN to std::nth_element), so the history never holds a NaN;
//   - a push whose time stamps do not strictly increase, or do not exceed the last one pushed, is refused as a whole with nothing done
//     (the reference refuses such images one by one);
//   - method 2 writes last_added and never reads it: it is not kept here.
// Every double operation below is a statement of its own and the unit is built with -ffp-contract=off: the roundings are the reference's.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "downsample_kernels.h"
#include "rir_amd_device.h"
#include "runtime.h"

using namespace rir;

namespace
{
	constexpr int HISTORY = 96;		// statistics the history holds at most (buffer_size, h264.cpp:206)
	constexpr int WARM_UP_2 = 10;	// method 2 decides on the grid alone until the history holds this many (h264.cpp:290)

	struct DecideState // all zero: a stream that has seen nothing
	{
		double history[HISTORY];
		int filled;
		int64_t seen;		// images so far (the reference's i)
		int64_t last_added; // method 1: the last image kept
		int64_t count;		// images kept so far
	};

	bool decide_args(int factor, double factor_std, int method, long long size)
	{
		return factor >= 1 && factor_std >= 0.0 && factor_std <= 1.0 && (method == 1 || method == 2) && size >= 2 && size <= 2147483647ll;
	}

	double statistic(int64_t sum_abs, int64_t sum_sq, long long size)
	{
		const double x = (double)sum_abs;
		const double q = (double)sum_sq;
		const double xx = x * x;
		const double m = xx / (double)size;
		const double r = q - m;
		if (r < 0.0)
			return 0.0;
		const double v = r / (double)(size - 1);
		return std::sqrt(v);
	}

	void mean_std(const double *p, int n, double &mean, double &std_dev)
	{
		double x = 0.0, x2 = 0.0;
		for (int i = 0; i < n; ++i)
		{
			const double sq = p[i] * p[i];
			x += p[i];
			x2 += sq;
		}
		mean = x / (double)n;
		const double xx = x * x;
		const double m = xx / (double)n;
		const double r = x2 - m;
		const double v = r / (double)(n - 1);
		std_dev = std::sqrt(v); // NaN for a negative radicand, as in the reference: every comparison it enters is then false
	}

	void push_history(DecideState &s, double stat)
	{
		if (s.filled < HISTORY)
			s.history[s.filled++] = stat;
		else
		{
			std::memmove(s.history, s.history + 1, (HISTORY - 1) * sizeof(double));
			s.history[HISTORY - 1] = stat;
		}
	}

	bool decide_method1(DecideState &s, int factor, int part, double stat)
	{
		const int64_t i = s.seen;
		if (s.filled < HISTORY)
		{
			if (i > 0)
				s.history[s.filled++] = stat;
			return i % factor == 0;
		}
		double sorted[HISTORY];
		std::memcpy(sorted, s.history, sizeof(sorted));
		std::nth_element(sorted, sorted + part, sorted + HISTORY);
		const double val = sorted[part];
		double mean, sd;
		mean_std(s.history, HISTORY, mean, sd);
		const double half = 0.5 * sd;
		const double low = mean - half;
		bool nothing = stat < low;
		if (i - s.last_added >= 2 * (int64_t)factor)
			nothing = false;
		const bool keep = (stat > val || i - s.last_added >= factor) && !nothing;
		const double ten = 10 * sd;
		const double high = mean + ten;
		if (stat < high)
			push_history(s, stat);
		return keep;
	}

	bool decide_method2(DecideState &s, int factor, double stat)
	{
		const int64_t i = s.seen;
		if (i == 0)
			return true;
		const bool grid = i % factor == 0;
		if (s.filled < WARM_UP_2)
		{
			s.history[s.filled++] = stat;
			return grid;
		}
		double mean, sd;
		mean_std(s.history, s.filled, mean, sd);
		const double ratio = sd / mean;
		const double two = 2 * sd;
		const double quiet = mean + two;
		const bool nothing = ratio < 0.1 && stat < quiet;
		const double half = 0.5 * sd;
		const double above = mean + half;
		const bool keep = grid || (!nothing && stat > above);
		const double five = 5 * sd;
		const double high = mean + five;
		const double low = mean - sd;
		if ((stat < high && stat > low) || grid)
			push_history(s, stat);
		return keep;
	}

	// The recurrence over n images whose sums are given; keep[i] = 1 for an image that triggers an output.  -> images kept
	int decide(DecideState &s, int factor, double factor_std, int method, long long size, const long long *sums, int n, int *keep, double *stats)
	{
		int part = (int)(factor_std * HISTORY);
		part = std::min(std::max(part, 0), HISTORY - 1);
		int kept = 0;
		for (int k = 0; k < n; ++k)
		{
			double stat = 0.0;
			bool take = true; // factor 1: every image goes through as it is
			if (factor != 1)
			{
				if (s.seen > 0)
					stat = statistic(sums[2 * k], sums[2 * k + 1], size);
				take = method == 1 ? decide_method1(s, factor, part, stat) : decide_method2(s, factor, stat);
				if (take && method == 1)
					s.last_added = s.seen;
			}
			keep[k] = take ? 1 : 0;
			if (stats)
				stats[k] = stat;
			kept += take ? 1 : 0;
			s.count += take ? 1 : 0;
			++s.seen;
		}
		return kept;
	}

	struct DownsamplerObject : public Object
	{
		const char *type_name() const override { return "Downsampler"; }
		int w = 0, h = 0, lossy_height = 0, factor = 1, method = 1;
		double factor_std = 0.0;
		DecideState state;
		bool any_stamp = false;
		long long last_stamp = 0;
		// device state: the last image pushed, and the running maximum in two buffers (a push reads one and writes the other)
		DeviceBuffer prev, held[2];
		int held_at = 0;	 // the buffer that holds the maximum
		bool holding = false; // images since the last kept one are in it
		DeviceBuffer sums, partials, segments;
		PinnedBuffer h_sums, h_segments;
		hipEvent_t done = nullptr; // behind the last push's work: the next push, on whatever stream, is ordered after it
		std::vector<int> keep;
		~DownsamplerObject() override
		{
			if (done)
			{
				(void)hipEventSynchronize(done);
				(void)hipEventDestroy(done);
			}
		}
	};

	bool overlap(const void *a, size_t abytes, const void *b, size_t bbytes)
	{
		const char *pa = (const char *)a, *pb = (const char *)b;
		return pa < pb + bbytes && pb < pa + abytes;
	}
} // namespace

RIR_EXPORT size_t rir_downsample_state_bytes(void) { return sizeof(DecideState); }

RIR_EXPORT int rir_downsample_decide(int factor, double factor_std, int method, long long size, const long long *sums, int n, void *state, int *keep,
									 double *stats)
{
	if (!decide_args(factor, factor_std, method, size) || n < 0 || !state || (n > 0 && (!sums || !keep)))
	{
		log_error("rir_downsample_decide: invalid argument (factor >= 1, factor_std in [0, 1], method 1 or 2, 2 <= size <= 2^31 - 1, n >= 0, "
				  "state, sums and keep given)");
		return -1;
	}
	DecideState s;
	std::memcpy(&s, state, sizeof(s));
	if (s.filled < 0 || s.filled > HISTORY || s.seen < 0)
	{
		log_error("rir_downsample_decide: the state is neither zeroed nor one this function wrote");
		return -1;
	}
	const int kept = decide(s, factor, factor_std, method, size, sums, n, keep, stats);
	std::memcpy(state, &s, sizeof(s));
	return kept;
}

RIR_EXPORT int rir_downsampler_create(int width, int height, int lossy_height, int factor, double factor_std, int method)
{
	if (width <= 0 || height <= 0 || lossy_height < 1 || lossy_height > height || (long long)width * height > 2147483647ll ||
		!decide_args(factor, factor_std, method, (long long)width * lossy_height))
	{
		log_error("rir_downsampler_create: invalid argument (width, height >= 1 with width * height < 2^31, 1 <= lossy_height <= height, "
				  "width * lossy_height >= 2, factor >= 1, factor_std in [0, 1], method 1 or 2)");
		return 0;
	}
	if (!device_ready())
		return 0;
	auto o = std::make_shared<DownsamplerObject>();
	o->w = width, o->h = height, o->lossy_height = lossy_height, o->factor = factor, o->factor_std = factor_std, o->method = method;
	std::memset(&o->state, 0, sizeof(o->state));
	const size_t bytes = (size_t)width * height * sizeof(uint16_t);
	if (!o->prev.reserve(bytes) || !o->held[0].reserve(bytes) || !o->held[1].reserve(bytes) ||
		!hip_ok(hipEventCreateWithFlags(&o->done, hipEventDisableTiming), "hipEventCreate"))
		return 0;
	return register_object(o);
}

RIR_EXPORT int rir_downsampler_count(int handle)
{
	auto o = lookup_as<DownsamplerObject>(handle);
	if (!o)
	{
		log_error("rir_downsampler_count: invalid handle");
		return -1;
	}
	return (int)o->state.count;
}

RIR_EXPORT void rir_downsampler_destroy(int handle)
{
	if (lookup_as<DownsamplerObject>(handle))
		remove_object(handle);
}

RIR_EXPORT int rir_downsampler_push_device(int handle, const unsigned short *d_frames, int nframes, const long long *timestamps, unsigned short *d_out,
										   int *positions, double *stats, void *stream)
{
	auto o = lookup_as<DownsamplerObject>(handle);
	if (!o || nframes < 0 || (nframes > 0 && (!d_frames || !timestamps || !d_out || !positions)))
	{
		log_error("rir_downsampler_push_device: invalid argument (a downsampler's handle, nframes >= 0, frames, time stamps, output and positions given)");
		return -1;
	}
	if (nframes == 0)
		return 0;
	if (o->factor != 1 && nframes > DS_MAX_FRAMES)
	{
		log_error("rir_downsampler_push_device: " + std::to_string(nframes) + " images in one push, at most " + std::to_string(DS_MAX_FRAMES) +
				  " (65535 slabs of " + std::to_string(DS_SLAB) + " for the pair sums): push the stack in pieces");
		return -1;
	}
	const size_t npx = (size_t)o->w * o->h, size = (size_t)o->w * o->lossy_height, image = npx * sizeof(uint16_t);
	for (int i = 0; i < nframes; ++i)
		if (i > 0 ? timestamps[i] <= timestamps[i - 1] : (o->any_stamp && timestamps[0] <= o->last_stamp))
		{
			log_error("rir_downsampler_push_device: the time stamps must increase strictly, from the last one pushed on");
			return -1;
		}
	if (overlap(d_frames, image * nframes, d_out, image * nframes))
	{
		log_error("rir_downsampler_push_device: the output overlaps the frames");
		return -1;
	}
	hipStream_t st = (hipStream_t)stream;
	// whatever stream the push before went to: its state (previous image, maximum, tables) is ready before this one touches it
	if (!hip_ok(hipStreamWaitEvent(st, o->done, 0), "hipStreamWaitEvent"))
		return -1;
	DecideState s = o->state;
	if ((int)o->keep.size() < nframes)
		o->keep.resize(nframes);
	int *keep = o->keep.data();
	if (o->factor == 1)
	{
		if (!hip_ok(hipMemcpyAsync(d_out, d_frames, image * nframes, hipMemcpyDeviceToDevice, st), "hipMemcpyAsync"))
			return -1;
		decide(s, 1, o->factor_std, o->method, (long long)size, nullptr, nframes, keep, stats);
		for (int i = 0; i < nframes; ++i)
			positions[i] = i;
		if (!hip_ok(hipEventRecord(o->done, st), "hipEventRecord"))
			return -1;
		o->state = s, o->any_stamp = true, o->last_stamp = timestamps[nframes - 1];
		return nframes;
	}
	// pass 1: the sums of every adjacent pair; the one wait of the call (it also serves the caller's queued work)
	const size_t table = (size_t)nframes * 2 * sizeof(int64_t);
	if (!o->sums.reserve(table) || !o->partials.reserve(downsample_partials_bytes((int64_t)size, nframes)) || !o->h_sums.reserve(table) ||
		!o->segments.reserve(((size_t)nframes + 1) * sizeof(DsSegment)) || !o->h_segments.reserve(((size_t)nframes + 1) * sizeof(DsSegment)))
		return -1;
	if (!hip_ok(launch_pair_sums(d_frames, s.seen > 0 ? o->prev.as<uint16_t>() : nullptr, (int64_t)npx, (int64_t)size, nframes,
								 o->partials.as<int64_t>(), o->sums.as<int64_t>(), st),
				"downsample pair sums") ||
		!hip_ok(hipMemcpyAsync(o->h_sums.ptr, o->sums.ptr, table, hipMemcpyDeviceToHost, st), "hipMemcpyAsync") ||
		!hip_ok(wait_stream(st), "downsample pair sums"))
		return -1;
	// the recurrence, and the kept images as segments of source frames
	const int kept = decide(s, o->factor, o->factor_std, o->method, (long long)size, o->h_sums.as<long long>(), nframes, keep, stats);
	DsSegment *segs = o->h_segments.as<DsSegment>();
	int nsegs = 0, start = 0;
	for (int i = 0; i < nframes; ++i)
		if (keep[i])
		{
			segs[nsegs] = DsSegment{start, i, nsegs, nsegs == 0 && o->holding ? 1 : 0};
			positions[nsegs++] = i;
			start = i + 1;
		}
	const bool open = start < nframes; // images after the last kept one: their maximum is carried
	if (open)
	{
		segs[nsegs] = DsSegment{start, nframes - 1, -1, nsegs == 0 && o->holding ? 1 : 0};
		++nsegs;
	}
	// pass 2: the kept images and the carried maximum; the last image stays for the next push's first pair
	if (!hip_ok(hipMemcpyAsync(o->segments.ptr, segs, (size_t)nsegs * sizeof(DsSegment), hipMemcpyHostToDevice, st), "hipMemcpyAsync") ||
		!hip_ok(launch_max_hold(d_frames, o->held[o->held_at].as<uint16_t>(), o->held[o->held_at ^ 1].as<uint16_t>(), d_out, (int64_t)npx,
								(int64_t)size, o->segments.as<DsSegment>(), nsegs, st),
				"downsample max-hold") ||
		!hip_ok(hipMemcpyAsync(o->prev.ptr, d_frames + (size_t)(nframes - 1) * npx, size * sizeof(uint16_t), hipMemcpyDeviceToDevice, st),
				"hipMemcpyAsync") ||
		!hip_ok(hipEventRecord(o->done, st), "hipEventRecord"))
		return -1;
	if (open)
		o->held_at ^= 1;
	o->holding = open;
	o->state = s, o->any_stamp = true, o->last_stamp = timestamps[nframes - 1];
	return kept;
}
