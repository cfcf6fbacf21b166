// The bounded-loss stream: host side of the loss injection of H264_Saver::addImageLossyNoCamera / addLoss (h264.cpp:2253-2607) on top of
// the kernels of lossy_kernels.hip - one stream's state (LossyState), its handle object (LossyObject), the step of a run of frames for
// one or many streams (lossy_step_streams, in stages) and the rir_lossy_* entry points.  The saver (video_io_abi.cpp) owns one
// LossyObject and sees it through lossy_stream.h.
#include <algorithm>
#include <cstring>

#include "lossy_stream.h"
#include "rir_amd_device.h"

using namespace rir;

extern "C"
{
	int rir_bad_pixels_create_device(const unsigned short *, int, int, void *);
	int rir_bad_pixels_correct_device(int, const unsigned short *, unsigned short *, int, void *);
	void bad_pixels_destroy(int);
}

namespace rir
{
	// ---- one stream's state --------------------------------------------------------------------
	LossyState::~LossyState()
	{
		if (bp_handle > 0)
			bad_pixels_destroy(bp_handle);
	}

	bool LossyState::prepare(int w_, int h_, int hl_, int running_average, bool subtract_min)
	{
		w = w_, h = h_, hl = std::max(0, std::min(hl_, h_));
		const size_t full = (size_t)w * h, s = (size_t)w * hl;
		const int ra = std::max(0, std::min(running_average, 64));
		if (!d_img.reserve(full * 2) || !d_tmp.reserve(full * 2) || !d_out.reserve(full * 2) || !d_ref.reserve(full * 2) ||
			!d_prev.reserve(full * 2) || !d_last.reserve(full * 2) || !d_sums.reserve(s * 4 + 4) || !d_cval.reserve(s * 2 + 4) ||
			!d_ccnt.reserve(s * 2 + 4) || !d_ring.reserve((size_t)std::max(ra, 1) * s * 2 + 4) || !d_hist.reserve(16384 * 4) ||
			!d_stats.reserve(8 * sizeof(long long)) || !d_min.reserve(4) || !d_budget.reserve(sizeof(LossyBudget)) ||
			!d_decision.reserve(sizeof(LossyDecision)) || !d_errs.reserve(2 * sizeof(int)) || !d_tickets.reserve(2 * sizeof(unsigned int)))
			return false;
		hipStream_t st = default_stream();
		// histogram, sums and budget start at zero; afterwards every frame leaves the first two cleared (lossy_kernels.hip)
		if (!hip_ok(hipMemsetAsync(d_sums.ptr, 0, s * 4 + 4, st), "memset") || !hip_ok(hipMemsetAsync(d_cval.ptr, 0, s * 2 + 4, st), "memset") ||
			!hip_ok(hipMemsetAsync(d_ccnt.ptr, 0, s * 2 + 4, st), "memset") || !hip_ok(hipMemsetAsync(d_hist.ptr, 0, 16384 * 4, st), "memset") ||
			!hip_ok(hipMemsetAsync(d_stats.ptr, 0, 8 * sizeof(long long), st), "memset") ||
			!hip_ok(hipMemsetAsync(d_budget.ptr, 0, sizeof(LossyBudget), st), "memset") ||
			!hip_ok(hipMemsetAsync(d_tickets.ptr, 0, 2 * sizeof(unsigned int), st), "memset"))
			return false;
		dev.refT = d_ref.as<uint16_t>(), dev.prevT = d_prev.as<uint16_t>(), dev.lastDL = d_last.as<uint16_t>();
		dev.ra_sums = d_sums.as<uint32_t>(), dev.ra_const_value = d_cval.as<uint16_t>(), dev.ra_const_count = d_ccnt.as<int16_t>();
		dev.ra_images = d_ring.as<uint16_t>();
		dev.ra_count = 0, dev.ra_head = 0, dev.running_average = ra;
		dev.subtract_min = subtract_min ? 1 : 0;
		dev.min = 0;
		frames = 0;
		return hip_ok(wait_stream(st), "sync"); // the state is ready whatever stream the steps run on
	}

	bool LossyState::step(const unsigned short *img, unsigned short *out, const LossyParams &p, int &low_error, int &high_error)
	{
		hipStream_t st = default_stream();
		const int full = w * h;
		int e[2] = {0, 0};
		if (!hip_ok(hipMemcpyAsync(d_img.ptr, img, (size_t)full * 2, hipMemcpyHostToDevice, st), "H2D") ||
			!queue_frame(d_img.as<uint16_t>(), d_out.as<uint16_t>(), p, d_errs.as<int>(), st) ||
			!hip_ok(hipMemcpyAsync(e, d_errs.ptr, sizeof(e), hipMemcpyDeviceToHost, st), "D2H"))
			return false;
		// (when out is NULL the caller consumes d_out on the same stream)
		if (out && !hip_ok(hipMemcpyAsync(out, d_out.ptr, (size_t)full * 2, hipMemcpyDeviceToHost, st), "D2H"))
			return false;
		if (!hip_ok(wait_stream(st), "sync"))
			return false;
		low_error = e[0], high_error = e[1];
		return true;
	}

	bool LossyState::queue_host_frame(const unsigned short *pinned_img, const LossyParams &p, int *d_errors)
	{
		hipStream_t st = default_stream();
		return hip_ok(hipMemcpyAsync(d_img.ptr, pinned_img, (size_t)w * h * 2, hipMemcpyHostToDevice, st), "H2D") &&
			   queue_frame(d_img.as<uint16_t>(), d_out.as<uint16_t>(), p, d_errors, st);
	}

	bool LossyState::queue_frame(const uint16_t *d_src, uint16_t *d_dst, const LossyParams &p, int *d_errors, hipStream_t st)
	{
		const int full = w * h, s = w * hl;
		const uint16_t *tmp = d_src; // without bad-pixel repair the frame is used as it is
		if (p.remove_bad_pixels && hl > 0)
		{ // bp.init on the first image (rows < lossy_height), bp.correct on every image (h264.cpp:2259-2266)
			if (frames == 0 && bp_handle <= 0)
				bp_handle = rir_bad_pixels_create_device(d_src, w, hl, st);
			uint16_t *fixed = d_tmp.as<uint16_t>();
			if (bp_handle <= 0 || rir_bad_pixels_correct_device(bp_handle, d_src, fixed, 1, st) != 0)
				return false;
			if (full > s && !hip_ok(hipMemcpyAsync(fixed + s, d_src + s, (size_t)(full - s) * 2, hipMemcpyDeviceToDevice, st), "D2D"))
				return false;
			tmp = fixed;
		}
		if (frames == 0)
		{
			if (dev.subtract_min && s > 0)
			{
				unsigned int mn = 65535;
				if (!hip_ok(launch_lossy_min(tmp, s, d_min.as<unsigned int>(), st), "lossy min") ||
					!hip_ok(hipMemcpyAsync(&mn, d_min.ptr, 4, hipMemcpyDeviceToHost, st), "D2H") || !hip_ok(wait_stream(st), "sync"))
					return false;
				dev.min = mn;
			}
			if (!hip_ok(launch_lossy_first(tmp, d_dst, dev, s, full, st), "lossy first"))
				return false;
			// the first image is stored as it is: its errors are the configured ones (h264.cpp:2290-2333)
			if (d_errors && (!hip_ok(hipMemsetD32Async((hipDeviceptr_t)d_errors, p.low, 1, st), "errors") ||
							 !hip_ok(hipMemsetD32Async((hipDeviceptr_t)(d_errors + 1), p.high, 1, st), "errors")))
				return false;
		}
		else
		{
			const LossyStep step = make_step(tmp, d_src, d_dst, p, d_errors);
			if (!hip_ok(launch_lossy_step(&step, nullptr, 1, st), "lossy step"))
				return false;
			advance_ring();
		}
		++frames;
		return true;
	}

	LossyStep LossyState::make_step(const uint16_t *tmp, const uint16_t *img, uint16_t *dst, const LossyParams &par, int *d_errors, int nstreams)
	{
		LossyStep p;
		p.hist_px = lossy_hist_px(w * hl, nstreams), p.reserved = 0;
		p.tmp = tmp, p.img = img, p.out = dst;
		p.st = dev;
		p.hist = d_hist.as<uint32_t>(), p.stats = d_stats.as<long long>();
		p.budget = d_budget.as<LossyBudget>(), p.decision = d_decision.as<LossyDecision>();
		p.errors_out = d_errors;
		p.tickets = d_tickets.as<unsigned int>();
		p.s = w * hl, p.full = w * h;
		p.add_loss = par.add_loss ? 1 : 0, p.low_value_error = par.low, p.high_value_error = par.high;
		p.std_factor = par.std_factor;
		p.next_tmp = p.next_img = nullptr, p.next_background = nullptr, p.next_errors_out = nullptr;
		p.do_update = 1, p.reserved2 = 0;
		return p;
	}

	bool LossyState::reserve_shadow()
	{
		if (shadow.refT)
			return true;
		const size_t full = (size_t)w * h, s = (size_t)w * hl;
		auto up = [](size_t v) { return (v + 255) / 256 * 256; };
		const size_t ring = (size_t)std::max(dev.running_average, 1) * s * 2 + 16;
		const size_t total = 3 * up(full * 2 + 16) + up(s * 4 + 16) + 2 * up(s * 2 + 16) + up(ring);
		if (!d_shadow.reserve(total))
			return false;
		char *p = d_shadow.as<char>();
		shadow = dev;
		shadow.refT = reinterpret_cast<uint16_t *>(p), p += up(full * 2 + 16);
		shadow.prevT = reinterpret_cast<uint16_t *>(p), p += up(full * 2 + 16);
		shadow.lastDL = reinterpret_cast<uint16_t *>(p), p += up(full * 2 + 16);
		shadow.ra_sums = reinterpret_cast<uint32_t *>(p), p += up(s * 4 + 16);
		shadow.ra_const_value = reinterpret_cast<uint16_t *>(p), p += up(s * 2 + 16);
		shadow.ra_const_count = reinterpret_cast<int16_t *>(p), p += up(s * 2 + 16);
		shadow.ra_images = reinterpret_cast<uint16_t *>(p);
		return true;
	}

	void LossyState::advance_ring()
	{
		if (dev.running_average > 0)
		{
			if (dev.ra_count == dev.running_average)
				dev.ra_head = (dev.ra_head + 1) % dev.running_average;
			else
				++dev.ra_count;
		}
	}

	// ---- the handle object -----------------------------------------------------------------------
	// What the run calls a stream LEADS keep between calls (every call's scratch is its leading stream's).
	struct LossyRunScratch
	{
		DeviceBuffer batch_errs;					// int[nframes][2] of the last rir_lossy_step_device call
		DeviceBuffer multi_table;					// rir_lossy_step_multi_device: the steps of the call (this object leads it)
		DeviceBuffer run_exchange;					// the run kernel's ticket, error word and exchange words
		DeviceBuffer run_hist, run_tickets, run_bg; // runs of frames: histogram slices and tickets of a group of frames, backgrounds of the call
		DeviceBuffer const_ok, const_partials;		// constant-budget form: one word per group of the last call (1 = stepped by it), the tail frames' sums
		int const_groups = 0;						// groups of the last run call that were OFFERED to the constant-budget form (0: it was not eligible)
		// speculative form (lossy_kernels.h: LossySpec): the budget tables, sums and statistics of a group (reused group after group), the control
		// words of every group and stream of the last call, and - for good - the back-off words of the calls this stream leads
		DeviceBuffer spec_budgets, spec_rows, spec_sd, spec_ctl, spec_backoff, spec_tickets, spec_dplane;
		PinnedBuffer spec_backoff_host;		   // the back-off words again, where the host can look without waiting (lossy_kernels.h: LossySpec::backoff_host)
		int spec_groups = 0, spec_streams = 0; // groups (and streams) of the last run call that went through the speculative launches (0: not eligible)
		PinnedBuffer multi_stage;
		hipEvent_t multi_copied = nullptr;			  // the copy out of multi_stage of the last call (whatever its stream) has completed
		unsigned int run_epoch = 0, run_arrivals = 0; // residency control block in run_exchange's header (resident_device.h): launches / workgroups so far
		std::vector<LossyParams> params;			  // what each stream of the call in progress is stepped under
		~LossyRunScratch()
		{
			if (multi_copied)
				(void)hipEventDestroy(multi_copied);
		}
		// the header of the exchange buffer (lossy_stream.h: kLossyRunErrorWord)
		unsigned int *ticket() { return run_exchange.as<unsigned int>(); }
		unsigned int *error_word() { return ticket() + kLossyRunErrorWord; }
		unsigned int *ctl() { return ticket() + kLossyRunCtlWord; } // arrivals, decision, poison, epoch of the first launch that bailed out
	};

	LossyObject::LossyObject() : scratch(new LossyRunScratch()) {}
	LossyObject::~LossyObject() {}

	LossyObject *LossyObject::leader()
	{
		if (lead_call == 0)
			return nullptr;
		if (!led_by_other)
			return this;
		// a foreign leader that is gone took its books with it: lead_call is a number of ITS numbering and must not be read against this
		// object's own ranges - "no record" (a call that was checked while its leader lived has filed its verdict with every member: is_failed())
		auto l = lead.lock();
		return l ? dynamic_cast<LossyObject *>(l.get()) : nullptr;
	}

	bool LossyObject::is_failed()
	{
		if (failed)
			return true;
		if (LossyObject *l = leader())
			for (const auto &r : l->led_bad)
				if (lead_call > r.first && lead_call <= r.second)
					failed = true;
		return failed;
	}

	bool LossyObject::has_run() const { return scratch->run_exchange.ptr != nullptr; }

	bool LossyObject::queue_verdict_read(unsigned int *words, hipStream_t st)
	{
		words[0] = words[1] = 0;
		return !has_run() || (hip_ok(hipMemcpyAsync(words, scratch->error_word(), 4, hipMemcpyDeviceToHost, st), "D2H") &&
							  hip_ok(hipMemcpyAsync(words + 1, scratch->ctl() + 2, 4, hipMemcpyDeviceToHost, st), "D2H"));
	}

	void LossyObject::checked(unsigned int gave_up, hipStream_t st)
	{
		if (gave_up)
		{
			led_bad.emplace_back(led_clean, led_calls);
			(void)hipMemsetAsync(scratch->error_word(), 0, 4, st);
		}
		led_clean = led_calls;
	}
} // namespace rir

// ---- the step of a run of frames, in stages ------------------------------------------------------------------------
// lossy_step_streams (at the end) is the sequence: switches, plan, scratch, tables, queue, read-back.  Only read_switches looks at the
// environment; only plan_call decides which form a call takes.
namespace
{
	// -- 1. switches: the environment of one call (read at every call: tests set them between calls) --
	struct LossySwitches
	{
		int max_workgroups;	  // RIR_LOSSY_RUN_MAX_WORKGROUPS (tests: a smaller limit, to go through the batches with small frames); <= 0: the device's
		bool form_set;		  // RIR_LOSSY_RUN_FORM=5 / 6: one form of the run kernel only, for tests and measurements
		int form;			  // ... its value
		bool per_frame;		  // RIR_LOSSY_LAUNCH_PER_FRAME
		bool no_const;		  // RIR_LOSSY_NO_CONST
		bool no_spec;		  // RIR_LOSSY_NO_SPEC
		int spec_passes;	  // RIR_LOSSY_SPEC_PASSES: 1 .. 16, 3 without it
		bool spec_first_only; // RIR_LOSSY_SPEC_FIRST_ONLY (comparison: a pass corrects the first wrong budget only - bit 8 of the launch's pass count)
		bool spec_no_give_up; // RIR_LOSSY_SPEC_NO_GIVE_UP (measurements: every pass that is allowed is made)
		bool spec_no_plane;	  // RIR_LOSSY_SPEC_NO_PLANE (measurements): no byte plane - the sums are taken from the frames, as they are when the memory is not to be had
		// (only in the build with the test hooks)
		int const_pairs; // RIR_LOSSY_CONST_PAIRS: the forms of the streaming kernel that small test frames would never take (0: chosen by the launch)
		bool give_up;	 // RIR_DEBUG_LOSSY_GIVE_UP (tests: as if a wait had hit its clock)
		int bail_group;	 // RIR_DEBUG_LOSSY_BAIL (tests: as if this group's launch had not become resident); -1: none
	};
	LossySwitches read_switches()
	{
		LossySwitches sw{};
		const char *max_env = getenv("RIR_LOSSY_RUN_MAX_WORKGROUPS");
		sw.max_workgroups = max_env ? atoi(max_env) : 0;
		const char *form = getenv("RIR_LOSSY_RUN_FORM");
		sw.form_set = form != nullptr, sw.form = form ? atoi(form) : 0;
		sw.per_frame = getenv("RIR_LOSSY_LAUNCH_PER_FRAME") != nullptr;
		sw.no_const = getenv("RIR_LOSSY_NO_CONST") != nullptr;
		sw.no_spec = getenv("RIR_LOSSY_NO_SPEC") != nullptr;
		const char *pe = getenv("RIR_LOSSY_SPEC_PASSES");
		sw.spec_passes = pe ? std::max(1, std::min(16, atoi(pe))) : 3;
		sw.spec_first_only = getenv("RIR_LOSSY_SPEC_FIRST_ONLY") != nullptr;
		sw.spec_no_give_up = getenv("RIR_LOSSY_SPEC_NO_GIVE_UP") != nullptr;
		sw.spec_no_plane = getenv("RIR_LOSSY_SPEC_NO_PLANE") != nullptr;
		const char *pairs = test_hook("RIR_LOSSY_CONST_PAIRS");
		sw.const_pairs = pairs ? atoi(pairs) : 0;
		sw.give_up = test_hook("RIR_DEBUG_LOSSY_GIVE_UP") != nullptr;
		const char *bail = test_hook("RIR_DEBUG_LOSSY_BAIL");
		sw.bail_group = bail ? atoi(bail) : -1;
		return sw;
	}

	// -- 2. plan: which form the call takes and how its tables lie, from numbers alone --
	struct LossyCall
	{
		int s_px, full_px;		   // pixels below lossy_height, pixels of a frame
		int nstreams, nsteps;	   // (nsteps: the frames of the call less the streams' very first)
		const LossyParams *params; // [nstreams]
		bool force_per_frame;	   // the second call of the recovery: no resident launch
	};
	struct LossyPlan
	{
		bool runs;		 // one launch per frame (lossy_frame_kernel) + one histogram launch per group of frames; false: three launches per step
		bool persistent; // the whole group of frames in one launch (lossy_run_kernel)
		bool parked;	 // ... in the kernel's second form
		int run_wgs;	 // workgroups of a stream in that launch
		int batch;		 // streams per launch of the resident kernel
		bool const_form, spec_form;
		int spec_passes; // passes of the speculative form, bit 8: first only, bit 9: no give-up
		int group, ngroups;
		size_t nfused, nhist, nbg; // entries of the per-frame table, of the histogram table behind it, backgrounds of the call
		size_t run_off, spec_off;  // where the LossyRun / LossySpec tables begin in the call's one table
		size_t nb;				   // bytes of that table
	};
	// capacity, capacity_parked: what THIS device holds of the run kernel's two forms at once (0: unknown)
	LossyPlan plan_call(const LossySwitches &sw, int capacity, int capacity_parked, const LossyCall &c)
	{
		LossyPlan p{};
		const int nstreams = c.nstreams, nsteps = c.nsteps;
		// runs: one launch per frame (lossy_frame_kernel) + one histogram launch per group of frames; needs whole groups of 8 pixels
		p.runs = nsteps >= 2 && c.s_px > 0 && c.s_px % 8 == 0 && c.full_px % 8 == 0;
		// persistent: the whole group of frames in one launch (lossy_run_kernel) when the chip holds a stream's workgroups at once
		p.run_wgs = lossy_run_workgroups(c.full_px);
		bool errors_fit = true; // (the run kernel hands a decision on as two 24-bit fields)
		for (int i = 0; i < nstreams; ++i)
			errors_fit = errors_fit && c.params[i].low < (1 << 24) && c.params[i].high < (1 << 24);
		// (more streams than the chip holds at once go through the resident kernel a batch of streams after the other: 6 streams of
		// 640x512 per launch keep 0.49 M frames/s whatever the number of streams; a launch per frame for all of them does 0.30-0.43 M)
		const int max_wgs = sw.max_workgroups > 0 ? std::min(sw.max_workgroups, capacity) : capacity;
		// the run kernel has a second form (part of the pixel state parked in LDS, one more wave per SIMD): more streams per launch, each
		// a little slower - taken when it saves a launch (runtime.h; RIR_LOSSY_RUN_FORM=5 / 6: one form only, for tests and measurements)
		const int max6 = sw.max_workgroups > 0 ? std::min(sw.max_workgroups, capacity_parked) : capacity_parked;
		const ResidentPlan plan = sw.form_set ? resident_plan(sw.form == 6 ? max6 : max_wgs, p.run_wgs, nstreams)
											  : resident_plan_two_forms(max_wgs, max6, p.run_wgs, nstreams, &p.parked);
		if (sw.form_set)
			p.parked = sw.form == 6; // (units_per_launch 0: a stream does not fit - launch per frame)
		p.persistent = p.runs && errors_fit && plan.units_per_launch > 0 && !c.force_per_frame && !sw.per_frame;
		// streams per launch of the resident kernel: the launches the plan needs, filled evenly (32 streams at 9 per launch: 8, 8, 8, 8 - not 9, 9, 9, 5)
		p.batch = p.persistent ? resident_batch(plan, nstreams) : nstreams;
		// The constant-budget form (lossy_kernels.hip: lossy_const_run_kernel): with stdFactor == 0 for every stream of the call each group is
		// first offered to an ordinary launch that needs no hand-offs between workgroups (decided on the device, group by group); it declines -
		// nothing waits for the host - when a frame's class may be empty or a NaN sits in a window, and the resident launch behind it, which
		// otherwise finds the group done and leaves, steps it.
		p.const_form = p.persistent && !sw.no_const;
		for (int i = 0; i < nstreams; ++i)
			p.const_form = p.const_form && c.params[i].std_factor == 0.0;
		// The speculative form (lossy_kernels.h: LossySpec): budgets that follow the statistics (stdFactor != 0, the reference's default) are guessed -
		// the configured errors, what a scene that does not move gets - and verified on the device; a group whose guess does not verify within
		// `spec_passes` corrections is left to the resident kernel, exactly as a declined constant-budget group is.
		p.spec_form = p.persistent && !p.const_form && !sw.no_spec;
		for (int i = 0; i < nstreams; ++i)
			p.spec_form = p.spec_form && c.params[i].low <= 65535 && c.params[i].high <= 65535; // (the budget table holds 16-bit fields)
		p.spec_passes = sw.spec_passes | (sw.spec_first_only ? 256 : 0) | (sw.spec_no_give_up ? 512 : 0);
		const bool stream_form = p.const_form || p.spec_form; // a streaming kernel steps whole groups: long ones
		// frames per histogram launch (one 64 KB histogram slice per frame and stream).  A group costs four small launches beside its
		// frames, so streams that may take the constant-budget form - 0.1 us per stream-frame - get groups four times as long (up to
		// 512 MB of slices, allocated as needed; 32 streams x 200 frames: 64-frame groups 0.83 M frames/s, one group 1.2 M)
		p.group = std::min(kLossyConstMaxFrames, std::max(1, (p.persistent ? (stream_form ? 8192 : 2048) : 512) / nstreams));
		// (the constant-budget kernel addresses a group's frames with 32-bit offsets below 2^31: groups of large frames are cut to fit -
		// 64 = the longest ring, 8 = the most frames it keeps in flight; lossy_const_run_kernel decides for itself, this only keeps it fast)
		if (stream_form)
			p.group = (int)std::max<long long>(1, std::min<long long>(p.group, 0x7fffffffll / ((long long)c.full_px * 2) - 64 - 8));
		p.ngroups = p.runs ? (nsteps + p.group - 1) / p.group : 0;
		// the descriptions of all launches of the call lie behind each other in one table
		// (the resident / constant-budget path takes its backgrounds straight from the runs' descriptions: no per-frame table)
		p.nfused = p.persistent ? 0 : p.runs ? (size_t)(nsteps + 1) * nstreams : (size_t)nsteps * nstreams;
		p.nbg = p.runs ? (size_t)nsteps * nstreams : 0;
		p.nhist = p.persistent ? 0 : p.nbg;
		p.run_off = (p.nfused + p.nhist) * sizeof(LossyStep); // (a multiple of 8)
		p.spec_off = p.run_off + (p.persistent ? (size_t)p.ngroups * nstreams * sizeof(LossyRun) : 0);
		static_assert(sizeof(LossyRun) % 8 == 0 && sizeof(LossySpec) % 8 == 0, "the tables of a call lie behind each other in one buffer");
		p.nb = p.spec_off + (p.persistent && p.spec_form ? (size_t)p.ngroups * nstreams * sizeof(LossySpec) : 0);
		return p;
	}

	// -- 3. scratch: the leading stream's buffers for the planned form --
	// scratch of the run kernel: [ticket, error word | 256 B][streams][2][run_wgs][slot_words] exchange words (zeroed before every launch)
	constexpr int kLossyRunSlotWords = 8;
	// workgroup 0 of a stream collects and decides (leader 0, every workgroup doing it, was measured slower at every stream count)
	constexpr int kLossyRunLeader = 1;
	// how the resident forms' buffers are divided among the streams of the call
	struct LossyRunLayout
	{
		size_t exch_words, exch_bytes; // exchange words of a stream / bytes of all streams' (behind the 256-byte header)
		size_t part_words;			   // constant-budget form: words of a stream's partial sums
		size_t spec_group;			   // speculative form: frames its per-group tables hold
		int spec_slabs;				   // ... slabs of a frame's sums
		bool spec_plane;			   // ... the byte plane (LossySpec::dplane) is to be had
	};
	// Reserves and, where a buffer grew, zeroes; the leader's books of rir_lossy_path_stats / rir_lossy_spec_stats are of THIS call, whatever path it takes.
	bool reserve_scratch(LossyRunScratch &sc, LossyObject *const *os, const LossyCall &c, const LossyPlan &p, bool no_plane, hipStream_t st, LossyRunLayout &L)
	{
		const int nstreams = c.nstreams;
		sc.const_groups = 0, sc.spec_groups = 0;
		// the descriptions of all launches of the call go to the device in one copy (page-locked staging: the copy is asynchronous
		// and the host buffer must outlive it - it is kept by the leading stream's object)
		if (!sc.multi_table.reserve(p.nb) || !sc.multi_stage.reserve(p.nb))
			return false;
		// an earlier call's copy out of the staging buffer may still be in flight - on whatever stream that call was given
		if (sc.multi_copied && !hip_ok(hipEventSynchronize(sc.multi_copied), "event"))
			return false;
		if (!sc.multi_copied && !hip_ok(hipEventCreateWithFlags(&sc.multi_copied, hipEventDisableTiming), "event"))
			return false;
		if (!p.runs)
			return true;
		// histogram scratch: one zeroed 16 384-bin slice and one ticket per frame of a group (the kernels leave them zeroed)
		const size_t slices = (size_t)std::min(c.nsteps, p.group) * nstreams;
		const size_t hist_cap = sc.run_hist.cap, tick_cap = sc.run_tickets.cap;
		if (!sc.run_hist.reserve(slices * 16384 * 4) || !sc.run_tickets.reserve(slices * 4) || !sc.run_bg.reserve(p.nbg * sizeof(long long)))
			return false;
		if (sc.run_hist.cap != hist_cap && !hip_ok(hipMemsetAsync(sc.run_hist.ptr, 0, sc.run_hist.cap, st), "memset"))
			return false;
		if (sc.run_tickets.cap != tick_cap && !hip_ok(hipMemsetAsync(sc.run_tickets.ptr, 0, sc.run_tickets.cap, st), "memset"))
			return false;
		if (!p.persistent)
			return true;
		L.exch_words = (size_t)2 * p.run_wgs * kLossyRunSlotWords + 16, L.exch_bytes = (size_t)nstreams * L.exch_words * 8;
		const size_t exch_cap = sc.run_exchange.cap;
		if (!sc.run_exchange.reserve(256 + L.exch_bytes))
			return false;
		if (sc.run_exchange.cap != exch_cap)
		{
			if (!hip_ok(hipMemsetAsync(sc.run_exchange.ptr, 0, 256, st), "memset"))
				return false;
			sc.run_arrivals = 0; // (a fresh control block)
		}
		L.part_words = (size_t)kLossyConstSlots * lossy_const_workgroups(c.full_px, nstreams) * 4;
		if (p.const_form)
		{
			if (!sc.const_ok.reserve((size_t)p.ngroups * 4) || !sc.const_partials.reserve((size_t)nstreams * L.part_words * 8) ||
				!hip_ok(hipMemsetAsync(sc.const_ok.ptr, 0, (size_t)p.ngroups * 4, st), "memset"))
				return false;
			sc.const_groups = p.ngroups;
		}
		L.spec_slabs = lossy_spec_stat_workgroups(c.s_px);
		L.spec_group = (size_t)std::min(c.nsteps, p.group);
		if (p.spec_form)
		{
			const size_t ng = (size_t)p.ngroups, sg = L.spec_group;
			const size_t bk_cap = sc.spec_backoff.cap, tk_cap = sc.spec_tickets.cap;
			if (!sc.const_ok.reserve(ng * 4) || !hip_ok(hipMemsetAsync(sc.const_ok.ptr, 0, ng * 4, st), "memset") ||
				!sc.spec_budgets.reserve((size_t)nstreams * (sg + 8) * 4) || !sc.spec_rows.reserve((size_t)nstreams * sg * L.spec_slabs * 32) ||
				!sc.spec_sd.reserve((size_t)nstreams * sg * 16) || !sc.spec_ctl.reserve(ng * nstreams * 32) ||
				!hip_ok(hipMemsetAsync(sc.spec_ctl.ptr, 0, ng * nstreams * 32, st), "memset") || !sc.spec_backoff.reserve(8) ||
				!sc.spec_tickets.reserve((size_t)nstreams * sg * 4))
				return false;
			// the byte plane the streaming kernel leaves for the sums kernel (lossy_kernels.h: LossySpec::dplane), a byte per pixel and frame of a group;
			// no_plane: none - the sums are taken from the frames, as they are when the memory is not to be had
			L.spec_plane = !no_plane && sc.spec_dplane.reserve((size_t)nstreams * sg * (size_t)c.s_px);
			if (sc.spec_tickets.cap != tk_cap && !hip_ok(hipMemsetAsync(sc.spec_tickets.ptr, 0, sc.spec_tickets.cap, st), "memset"))
				return false;
			if (sc.spec_backoff.cap != bk_cap && !hip_ok(hipMemsetAsync(sc.spec_backoff.ptr, 0, 8, st), "memset"))
				return false;
			if (!sc.spec_backoff_host.ptr)
			{
				if (!sc.spec_backoff_host.reserve(64))
					return false;
				std::memset(sc.spec_backoff_host.ptr, 0, 64);
			}
			for (int i = 0; i < nstreams; ++i)
				if (!os[i]->st.reserve_shadow())
					return false;
			sc.spec_groups = p.ngroups, sc.spec_streams = nstreams;
		}
		return true;
	}

	// -- 4. tables: one builder per form fills the staging buffer and advances the host side of every stream's state --
	// the frames of the call: frame f of stream i, and where its budget goes on the device
	struct LossyFrames
	{
		const unsigned short *const *d_in;
		unsigned short *const *d_out;
		int *const *d_errs; // the caller's arrays, or NULL
		int *own_errs;		// the call's own array (read back at the end), or NULL
		size_t npx;
		int nframes, f0; // f0: the first frame that is a step (1 when the call brought the streams' very first frame)
		const unsigned short *in(int i, size_t f) const { return d_in[i] + f * npx; }
		unsigned short *out(int i, size_t f) const { return d_out[i] + f * npx; }
		// the caller's array, the call's own, or nowhere
		int *errs_of(int i, int f) const { return d_errs ? d_errs[i] + (size_t)f * 2 : own_errs ? own_errs + ((size_t)i * nframes + f) * 2 : (int *)nullptr; }
	};

	// three launches per step: entry [step][stream]
	void build_step_table(LossyStep *hs, LossyObject *const *os, const LossyCall &c, const LossyFrames &fr)
	{
		for (int f = fr.f0; f < fr.nframes; ++f)
			for (int i = 0; i < c.nstreams; ++i)
			{
				LossyState &ls = os[i]->st;
				hs[(size_t)(f - fr.f0) * c.nstreams + i] = ls.make_step(fr.in(i, f), fr.in(i, f), fr.out(i, f), c.params[i], fr.errs_of(i, f), c.nstreams);
				ls.advance_ring();
				++ls.frames;
			}
	}

	// a launch per frame: entry [launch][stream], and behind them the histogram entries [frame][stream]
	void build_frame_table(LossyStep *hs, LossyRunScratch &sc, LossyObject *const *os, const LossyCall &c, const LossyPlan &p, const LossyFrames &fr)
	{
		const int nstreams = c.nstreams, nsteps = c.nsteps, group = p.group;
		long long *bg = sc.run_bg.as<long long>();
		LossyStep *hh = hs + p.nfused;
		for (int k = 0; k <= nsteps; ++k) // launch k updates frame f0 + k - 1 (k > 0) and takes the sums of frame f0 + k (k < nsteps)
			for (int i = 0; i < nstreams; ++i)
			{
				LossyState &ls = os[i]->st;
				LossyStep s;
				if (k == 0)
				{
					s = ls.make_step(nullptr, nullptr, nullptr, c.params[i], nullptr, nstreams);
					s.do_update = 0;
				}
				else
				{
					const size_t f = (size_t)(fr.f0 + k - 1);
					s = ls.make_step(fr.in(i, f), fr.in(i, f), fr.out(i, f), c.params[i], nullptr, nstreams);
					ls.advance_ring();
					++ls.frames;
				}
				if (k < nsteps)
				{
					const size_t fn = (size_t)(fr.f0 + k);
					s.next_tmp = s.next_img = fr.in(i, fn);
					s.next_background = bg + (size_t)k * nstreams + i;
					s.next_errors_out = fr.errs_of(i, (int)fn);
					LossyStep h{};
					const int in_group = std::min(group, nsteps - k / group * group);
					const size_t slice = (size_t)(k % group) * nstreams + i;
					h.tmp = h.img = fr.in(i, fn);
					h.hist = sc.run_hist.as<uint32_t>() + slice * 16384;
					h.stats = bg + (size_t)k * nstreams + i;
					h.tickets = sc.run_tickets.as<unsigned int>() + slice;
					h.s = c.s_px, h.full = c.full_px;
					h.hist_px = lossy_hist_px(c.s_px, in_group * nstreams);
					hh[(size_t)k * nstreams + i] = h;
				}
				hs[(size_t)k * nstreams + i] = s;
			}
	}

	// the host side of a stream's state as it was before a group - what a launch that did not become resident (it has written nothing) is repeated from
	struct LossySnap
	{
		int ra_count, ra_head;
		int64_t frames;
	};
	// resident forms: the LossyRun (and LossySpec) of every group and stream, entry [group][stream]; snaps: [ngroups][nstreams]
	void build_run_tables(char *stage, LossyRunScratch &sc, LossyObject *const *os, const LossyCall &c, const LossyPlan &p, const LossyRunLayout &L, const LossyFrames &fr,
						  std::vector<LossySnap> &snaps)
	{
		const int nstreams = c.nstreams;
		long long *bg = sc.run_bg.as<long long>();
		unsigned long long *d_exch = reinterpret_cast<unsigned long long *>(sc.run_exchange.as<char>() + 256);
		LossyRun *hr = reinterpret_cast<LossyRun *>(stage + p.run_off);
		LossySpec *hsp = reinterpret_cast<LossySpec *>(stage + p.spec_off);
		for (int g = 0; g < p.ngroups; ++g)
		{
			const int k0 = g * p.group, in_group = std::min(p.group, c.nsteps - k0);
			for (int i = 0; i < nstreams; ++i)
			{
				LossyState &ls = os[i]->st;
				const LossyParams &par = c.params[i];
				snaps.push_back(LossySnap{ls.dev.ra_count, ls.dev.ra_head, (int64_t)ls.frames});
				LossyRun r{};
				r.in = fr.in(i, (size_t)(fr.f0 + k0)), r.out = fr.out(i, (size_t)(fr.f0 + k0));
				r.st = ls.dev;
				r.bg = bg + (size_t)k0 * nstreams + i, r.bg_stride = nstreams;
				r.budget = ls.d_budget.as<LossyBudget>(), r.decision = ls.d_decision.as<LossyDecision>();
				r.errors_out = fr.errs_of(i, fr.f0 + k0);
				r.exchange = d_exch + (size_t)i * L.exch_words, r.error_word = sc.error_word(), r.slot_words = kLossyRunSlotWords, r.leader = kLossyRunLeader;
				r.frame_px = (long long)fr.npx, r.nsteps = in_group;
				r.s = c.s_px, r.full = c.full_px;
				r.add_loss = par.add_loss ? 1 : 0, r.low_value_error = par.low, r.high_value_error = par.high, r.std_factor = par.std_factor;
				r.partials = p.const_form ? sc.const_partials.as<unsigned long long>() + (size_t)i * L.part_words : nullptr;
				hr[(size_t)g * nstreams + i] = r;
				if (p.spec_form)
				{
					LossySpec sp{};
					sp.shadow = ls.shadow;
					sp.shadow.ra_count = ls.dev.ra_count, sp.shadow.ra_head = ls.dev.ra_head, sp.shadow.running_average = ls.dev.running_average;
					sp.budgets = sc.spec_budgets.as<uint32_t>() + (size_t)i * (L.spec_group + 8);
					sp.rows = sc.spec_rows.as<unsigned long long>() + (size_t)i * L.spec_group * L.spec_slabs * 4;
					sp.sd = sc.spec_sd.as<double>() + (size_t)i * L.spec_group * 2;
					sp.tickets = sc.spec_tickets.as<unsigned int>() + (size_t)i * L.spec_group;
					sp.ctl = sc.spec_ctl.as<unsigned int>() + ((size_t)g * nstreams + i) * 8;
					sp.backoff = sc.spec_backoff.as<unsigned int>();
					sp.backoff_host = sc.spec_backoff_host.as<unsigned int>();
					sp.dplane = L.spec_plane ? sc.spec_dplane.as<uint8_t>() + (size_t)i * L.spec_group * (size_t)c.s_px : nullptr;
					hsp[(size_t)g * nstreams + i] = sp;
				}
				for (int k = k0; k < k0 + in_group; ++k)
				{ // (the host side of the stream's state as it will be after the group)
					ls.advance_ring();
					++ls.frames;
				}
			}
		}
	}

	// the call's table to the device in one copy, and the event that says the staging buffer is free again
	bool copy_tables(LossyRunScratch &sc, size_t nb, hipStream_t st)
	{
		return hip_ok(hipMemcpyAsync(sc.multi_table.ptr, sc.multi_stage.ptr, nb, hipMemcpyHostToDevice, st), "H2D") && hip_ok(hipEventRecord(sc.multi_copied, st), "event");
	}

	// -- 5. queue: one function per form issues the launches --
	bool queue_steps(LossyRunScratch &sc, const LossyCall &c, hipStream_t st)
	{
		const LossyStep *hs = sc.multi_stage.as<LossyStep>(), *dt = sc.multi_table.as<LossyStep>();
		for (int f = 0; f < c.nsteps; ++f)
			if (!hip_ok(launch_lossy_step(hs + (size_t)f * c.nstreams, dt + (size_t)f * c.nstreams, c.nstreams, st), "lossy step"))
				return false;
		return true;
	}

	bool queue_frames(LossyRunScratch &sc, const LossyCall &c, const LossyPlan &p, hipStream_t st)
	{
		const LossyStep *dt = sc.multi_table.as<LossyStep>();
		for (int k = 0; k <= c.nsteps; ++k)
		{
			if (k < c.nsteps && k % p.group == 0)
			{
				const int in_group = std::min(p.group, c.nsteps - k);
				if (!hip_ok(launch_lossy_backgrounds(dt + p.nfused + (size_t)k * c.nstreams, in_group * c.nstreams, c.s_px, lossy_hist_px(c.s_px, in_group * c.nstreams), st),
							"lossy backgrounds"))
					return false;
			}
			if (!hip_ok(launch_lossy_frame(dt + (size_t)k * c.nstreams, c.nstreams, c.full_px, st), "lossy frame"))
				return false;
		}
		return true;
	}

	// the speculative launches of group g: guess, (step, sums, verify) x passes, commit - every launch returns at once when the one before left it nothing to do
	bool queue_spec_group(LossyRunScratch &sc, const LossyCall &c, const LossyPlan &p, const LossyRun *dr, const LossySpec *dsp, int g, int in_group, bool any_ra, hipStream_t st)
	{
		unsigned int *d_ok = sc.const_ok.as<unsigned int>() + g;
		const bool add_loss = c.params[0].add_loss;
		if (!hip_ok(launch_lossy_spec_begin(dr, dsp, c.nstreams, p.spec_passes, d_ok, sc.ctl() + 2, st), "lossy speculative run"))
			return false;
		for (int pass = 0; pass < (p.spec_passes & 0xff); ++pass)
			if (!hip_ok(launch_lossy_spec_pass(dr, dsp, c.nstreams, c.s_px, c.full_px, in_group, any_ra, add_loss, st), "lossy speculative pass"))
				return false;
		return hip_ok(launch_lossy_spec_commit(dr, dsp, c.nstreams, c.s_px, c.full_px, d_ok, st), "lossy speculative commit");
	}

	// Resident forms.  run_epochs: [ngroups] the epoch of each group's first resident launch (resident_device.h) - what the read-back finds the group
	// that bailed by.  give_up, bail_group: the test hooks (LossySwitches).
	bool queue_runs(LossyObject &lead, LossyObject *const *os, const LossyCall &c, const LossyPlan &p, const LossyRunLayout &L, bool give_up, int bail_group, hipStream_t st,
					std::vector<unsigned int> &run_epochs)
	{
		LossyRunScratch &sc = *lead.scratch;
		const int nstreams = c.nstreams;
		const bool add_loss = c.params[0].add_loss; // (the same for all streams of a call)
		unsigned int *d_ticket = sc.ticket();
		unsigned long long *d_exch = reinterpret_cast<unsigned long long *>(sc.run_exchange.as<char>() + 256);
		const LossyRun *dr = reinterpret_cast<const LossyRun *>(sc.multi_table.as<char>() + p.run_off);
		const LossySpec *dsp = reinterpret_cast<const LossySpec *>(sc.multi_table.as<char>() + p.spec_off);
		// the call is on the leader's books before anything is queued: whatever happens from here on, a raised error word
		// is charged to it
		++lead.led_calls;
		for (int i = 0; i < nstreams; ++i)
		{
			os[i]->lead_call = lead.led_calls;
			os[i]->led_by_other = i != 0;
			if (i == 0)
				os[i]->lead.reset();
			else
				os[i]->lead = lead.weak_from_this();
		}
		if (give_up && !hip_ok(hipMemsetAsync(sc.error_word(), 1, 4, st), "memset")) // (tests: as if a wait had hit its clock)
			return false;
		// A stream that backs off (its groups kept failing: budgets that move) is not offered its next groups: the device's counter says how
		// many, the host looks at its page-locked copy - without waiting, so the value may be a call or two old: then fewer groups are left
		// out here and the device skips them itself - and does not even queue their launches (eleven small ones per group).
		int host_skipped = 0;
		if (p.spec_form)
		{
			const unsigned int left = *reinterpret_cast<volatile unsigned int *>(sc.spec_backoff_host.ptr);
			host_skipped = (int)std::min<unsigned int>(left, (unsigned int)p.ngroups);
			if (host_skipped > 0 &&
				!hip_ok(launch_lossy_spec_skipped(sc.spec_backoff.as<unsigned int>(), sc.spec_backoff_host.as<unsigned int>(), (unsigned int)host_skipped, st), "lossy speculative skip"))
				return false;
		}
		bool any_ra = false;
		for (int i = 0; i < nstreams; ++i)
			any_ra = any_ra || os[i]->st.dev.running_average > 0;
		for (int g = 0; g < p.ngroups; ++g)
		{
			const int k0 = g * p.group, in_group = std::min(p.group, c.nsteps - k0);
			const LossyRun *drg = dr + (size_t)g * nstreams;
			if (!hip_ok(launch_lossy_backgrounds_of_runs(drg, nstreams, in_group, sc.run_hist.as<uint32_t>(), sc.run_tickets.as<unsigned int>(), c.s_px,
														 lossy_hist_px(c.s_px, in_group * nstreams), st),
						"lossy backgrounds") ||
				!hip_ok(hipMemsetAsync(d_exch, 0, L.exch_bytes, st), "memset"))
				return false;
			// (a streaming form's word for the group: the resident launch behind it leaves the group alone when it says 1)
			const unsigned int *d_ok = p.const_form || p.spec_form ? sc.const_ok.as<unsigned int>() + g : nullptr;
			if (p.const_form && !hip_ok(launch_lossy_const(drg, nstreams, c.full_px, any_ra, add_loss, sc.const_ok.as<unsigned int>() + g, sc.ctl() + 2, st), "lossy constant-budget run"))
				return false;
			if (p.spec_form && g >= host_skipped && !queue_spec_group(sc, c, p, drg, dsp + (size_t)g * nstreams, g, in_group, any_ra, st))
				return false;
			for (int s0 = 0; s0 < nstreams; s0 += p.batch)
			{
				const int nl = std::min(p.batch, nstreams - s0);
				const unsigned int epoch = ++sc.run_epoch;
				if (s0 == 0)
					run_epochs.push_back(epoch);
				if (bail_group == g)
				{ // (tests: as if group g's launch had not become resident: its decision is BAIL before anybody arrives)
					const unsigned int w_ = ((epoch & 0x3fffffffu) << 2) | 2u;
					if (!hip_ok(hipMemcpyAsync(sc.ctl() + 1, &w_, 4, hipMemcpyHostToDevice, st), "H2D") || !hip_ok(hipStreamSynchronize(st), "sync"))
						return false;
				}
				if (!hip_ok(launch_lossy_run(drg + s0, nl, c.full_px, d_ticket, epoch, sc.run_arrivals, p.parked, st, d_ok), "lossy run"))
					return false;
				sc.run_arrivals += (unsigned int)(nl * p.run_wgs);
			}
		}
		return true;
	}

	// -- 6. read-back and recovery: the budgets and the verdict of a call that returns budgets --
	// what the resident launches of the call left for it (empty / 0 for the other forms)
	struct LossyRunTrace
	{
		std::vector<unsigned int> run_epochs; // [ngroups]: epoch of the group's first launch
		std::vector<LossySnap> snaps;		  // [ngroups][nstreams]
		int group = 0, launches_per_group = 0;
	};
	int read_back(LossyObject *const *os, int nstreams, const LossyFrames &fr, int add_loss, const LossyRunTrace &tr, int *low_errors, int *high_errors, hipStream_t st)
	{
		LossyObject &lead = *os[0];
		LossyRunScratch &sc = *lead.scratch;
		const int nframes = fr.nframes;
		std::vector<int> e((size_t)nstreams * nframes * 2);
		unsigned int gave_up = 0;			// the run kernel's error word (a wait between workgroups that hit its clock)
		unsigned int ctl[4] = {0, 0, 0, 0}; // the residency control block: arrivals, decision, poison, epoch of the first launch that bailed out
		if ((lead.has_run() && (!hip_ok(hipMemcpyAsync(&gave_up, sc.error_word(), 4, hipMemcpyDeviceToHost, st), "D2H") ||
								!hip_ok(hipMemcpyAsync(ctl, sc.ctl(), sizeof(ctl), hipMemcpyDeviceToHost, st), "D2H"))) ||
			!hip_ok(wait_stream(st), "sync"))
			return -1;
		if (ctl[2] != 0 && !tr.run_epochs.empty())
		{
			// A group's launch did not become resident (ordinary kernels of other streams can keep the last workgroups from fitting:
			// resident_device.h).  It and every launch behind it have written nothing.  The call waits here anyway, so the frames
			// from that group on are stepped again on the launch-per-frame path - same results - from the host state of that moment.
			int g_bad = -1;
			for (size_t g = 0; g < tr.run_epochs.size(); ++g)
				if (g_bad < 0 && (int)(ctl[3] - tr.run_epochs[g]) >= 0 && (int)(ctl[3] - tr.run_epochs[g]) < tr.launches_per_group)
					g_bad = (int)g;
			const unsigned int zero2[2] = {0, 0};
			if (!hip_ok(hipMemcpyAsync(sc.ctl() + 2, zero2, sizeof(zero2), hipMemcpyHostToDevice, st), "H2D") || !hip_ok(hipStreamSynchronize(st), "sync"))
				return -1;
			if (g_bad < 0 || tr.launches_per_group != 1)
			{ // (a poison left by an earlier, queue-only call - or streams that went in several batches and stand at different frames)
				gave_up = 1;
			}
			else
			{
				const int fr0 = fr.f0 + g_bad * tr.group; // first frame that was not stepped
				for (int i = 0; i < nstreams; ++i)
				{
					const LossySnap &sn = tr.snaps[(size_t)g_bad * nstreams + i];
					os[i]->st.dev.ra_count = sn.ra_count, os[i]->st.dev.ra_head = sn.ra_head, os[i]->st.frames = (decltype(os[i]->st.frames))sn.frames;
				}
				std::vector<const unsigned short *> in2((size_t)nstreams);
				std::vector<unsigned short *> out2((size_t)nstreams);
				std::vector<int *> errs2((size_t)nstreams);
				for (int i = 0; i < nstreams; ++i)
				{
					in2[i] = fr.in(i, (size_t)fr0), out2[i] = fr.out(i, (size_t)fr0);
					errs2[i] = sc.batch_errs.as<int>() + ((size_t)i * nframes + fr0) * 2;
				}
				if (lossy_step_streams(os, nstreams, in2.data(), out2.data(), nframes - fr0, add_loss, errs2.data(), nullptr, nullptr, st, true) != 0 ||
					!hip_ok(wait_stream(st), "sync"))
					return -1;
			}
		}
		if (!hip_ok(hipMemcpyAsync(e.data(), sc.batch_errs.ptr, e.size() * sizeof(int), hipMemcpyDeviceToHost, st), "D2H") || !hip_ok(wait_stream(st), "sync"))
			return -1;
		if (lead.has_run())
			lead.checked(gave_up, st);
		bool any_failed = false;
		for (int i = 0; i < nstreams; ++i)
			any_failed = os[i]->is_failed() || any_failed; // (every stream of the call is marked)
		if (any_failed)
		{
			log_error("rir_lossy_step_multi_device: a run of frames gave up waiting (results invalid; the streams of the call take no more frames)");
			return -1;
		}
		for (size_t i = 0; i < (size_t)nstreams * nframes; ++i)
		{
			if (low_errors)
				low_errors[i] = e[2 * i];
			if (high_errors)
				high_errors[i] = e[2 * i + 1];
		}
		return 0;
	}
} // namespace

namespace rir
{
	int lossy_step_streams(LossyObject *const *os, int nstreams, const unsigned short *const *d_in, unsigned short *const *d_out, int nframes, int add_loss,
						   int *const *d_errs, int *low_errors, int *high_errors, hipStream_t st, bool force_per_frame)
	{
		const bool want = low_errors || high_errors;
		LossyObject &lead = *os[0]; // owns the scratch of the call: the table of steps and the budgets
		LossyRunScratch &sc = *lead.scratch;
		for (int i = 0; i < nstreams; ++i)
			if (os[i]->is_failed())
			{
				log_error("bounded-loss step: a run of frames of this stream gave up earlier - its state is invalid, destroy the stream");
				return -1;
			}
		if (want && !d_errs && !sc.batch_errs.reserve((size_t)nstreams * nframes * 2 * sizeof(int)))
			return -1;
		sc.params.resize((size_t)nstreams);
		for (int i = 0; i < nstreams; ++i)
		{
			sc.params[i] = os[i]->params(add_loss != 0);
			sc.params[i].remove_bad_pixels = false; // (checked by the callers)
		}
		LossyFrames fr{d_in, d_out, d_errs, want && !d_errs ? sc.batch_errs.as<int>() : nullptr, (size_t)os[0]->st.w * os[0]->st.h, nframes, 0};
		if (os[0]->st.frames == 0)
		{ // first frame of every stream: stored as it is, seeds the state - one small launch per stream, once in a stream's life
			for (int i = 0; i < nstreams; ++i)
				if (!os[i]->st.queue_frame(d_in[i], d_out[i], sc.params[i], fr.errs_of(i, 0), st))
					return -1;
			fr.f0 = 1;
		}
		LossyRunTrace tr;
		const LossyCall c{os[0]->st.w * os[0]->st.hl, os[0]->st.w * os[0]->st.h, nstreams, nframes - fr.f0, sc.params.data(), force_per_frame};
		if (c.nsteps > 0)
		{
			const LossySwitches sw = read_switches();
			lossy_const_force_pairs(sw.const_pairs); // (before anything is sized: lossy_const_workgroups follows it)
			const LossyPlan p = plan_call(sw, lossy_run_capacity(), lossy_run_capacity(true), c);
			LossyRunLayout L{};
			if (!reserve_scratch(sc, os, c, p, sw.spec_no_plane, st, L))
				return -1;
			if (!p.runs)
				build_step_table(sc.multi_stage.as<LossyStep>(), os, c, fr);
			else if (p.persistent)
				build_run_tables(sc.multi_stage.as<char>(), sc, os, c, p, L, fr, tr.snaps);
			else
				build_frame_table(sc.multi_stage.as<LossyStep>(), sc, os, c, p, fr);
			if (!copy_tables(sc, p.nb, st))
				return -1;
			if (!(!p.runs ? queue_steps(sc, c, st) : p.persistent ? queue_runs(lead, os, c, p, L, sw.give_up, sw.bail_group, st, tr.run_epochs) : queue_frames(sc, c, p, st)))
				return -1;
			if (p.persistent)
				tr.group = p.group, tr.launches_per_group = (nstreams + p.batch - 1) / p.batch;
		}
		if (want && !d_errs)
			return read_back(os, nstreams, fr, add_loss, tr, low_errors, high_errors, st);
		return 0;
	}
} // namespace rir

// ---- bounded-loss step on a device-resident stream ---------------------------------------------------------------
// The loss injection of H264_Saver::addImageLossyNoCamera / addLoss (h264.cpp:2253-2607) without the saver around it:
// frames in HBM in, frames in HBM out, one state object per stream.
RIR_EXPORT int rir_lossy_create(int width, int height, int lossy_height, int low_value_error, int high_value_error, double std_factor,
								int running_average, int subtract_min, int remove_bad_pixels)
{
	if (!device_ready())
		return 0;
	if (width <= 0 || height <= 0 || lossy_height < 0)
	{
		log_error("rir_lossy_create: invalid argument");
		return 0;
	}
	auto o = std::make_shared<LossyObject>();
	o->low = low_value_error, o->high = high_value_error, o->std_factor = std_factor, o->remove_bad_pixels = remove_bad_pixels != 0;
	if (!o->st.prepare(width, height, lossy_height, running_average, subtract_min != 0))
		return 0;
	return register_object(o);
}

// A parameter change on a stream in use (H264_Saver::setParameter lowValueError / highValueError / stdFactor, h264.cpp:1709-1781): applies
// from the next frame on; the history the budget is computed from (firstStdDevs, the 40-frame window) stays.
RIR_EXPORT int rir_lossy_set_errors(int handle, int low_value_error, int high_value_error, double std_factor)
{
	auto o = lookup_as<LossyObject>(handle);
	if (!o)
	{
		log_error("rir_lossy_set_errors: invalid handle");
		return -1;
	}
	o->low = low_value_error, o->high = high_value_error, o->std_factor = std_factor;
	return 0;
}

// (the runs of frames read input frames again - the frame that leaves the running average - after later outputs have been written)
static bool frames_overlap(const char *who, const LossyState &s, const unsigned short *d_in, const unsigned short *d_out, int nframes)
{
	const size_t span = (size_t)nframes * (size_t)s.w * (size_t)s.h;
	if (!(d_in < d_out + span && d_out < d_in + span))
		return false;
	log_error(std::string(who) + ": input and output frames overlap");
	return true;
}

// d_in, d_out: uint16 [nframes][height][width], distinct buffers; low_errors / high_errors: HOST int[nframes] (may be NULL).
// Frames are processed in order (the state is sequential); add_loss != 0 selects the addLoss variant.
RIR_EXPORT int rir_lossy_step_device(int handle, const unsigned short *d_in, unsigned short *d_out, int nframes, int add_loss, int *low_errors,
									 int *high_errors, void *stream)
{
	auto o = lookup_as<LossyObject>(handle);
	if (!o || !d_in || !d_out || d_in == d_out || nframes <= 0)
	{
		log_error("rir_lossy_step_device: invalid argument");
		return -1;
	}
	if (frames_overlap("rir_lossy_step_device", o->st, d_in, d_out, nframes))
		return -1;
	// a batch without bad-pixel repair is a run of frames: one launch per frame instead of three (rir_lossy_step_multi_device)
	if (!o->remove_bad_pixels && nframes >= 3)
	{
		const unsigned short *in1[1] = {d_in};
		unsigned short *out1[1] = {d_out};
		return rir_lossy_step_multi_device(&handle, 1, in1, out1, nframes, add_loss, low_errors, high_errors, stream);
	}
	// every frame is queued without waiting (statistics, budget and update all run on the device); the budgets of the batch
	// come back in one copy at the end - or not at all when the caller does not ask for them: then nothing here waits
	const size_t npx = (size_t)o->st.w * o->st.h;
	hipStream_t st = (hipStream_t)stream;
	const bool want = low_errors || high_errors;
	DeviceBuffer &batch_errs = o->scratch->batch_errs;
	if (want && !batch_errs.reserve((size_t)nframes * 2 * sizeof(int)))
		return -1;
	const LossyParams par = o->params(add_loss != 0);
	for (int i = 0; i < nframes; ++i)
		if (!o->st.queue_frame(d_in + (size_t)i * npx, d_out + (size_t)i * npx, par, want ? batch_errs.as<int>() + 2 * i : nullptr, st))
			return -1;
	if (want)
	{
		std::vector<int> e((size_t)nframes * 2);
		if (!hip_ok(hipMemcpyAsync(e.data(), batch_errs.ptr, e.size() * sizeof(int), hipMemcpyDeviceToHost, st), "D2H") ||
			!hip_ok(wait_stream(st), "sync"))
			return -1;
		for (int i = 0; i < nframes; ++i)
		{
			if (low_errors)
				low_errors[i] = e[2 * i];
			if (high_errors)
				high_errors[i] = e[2 * i + 1];
		}
	}
	return 0;
}

// The same step for `nstreams` INDEPENDENT streams (one state object each, equal geometry and history length) with the streams
// sharing every launch: frame f of all streams = three launches whose grids carry the stream in their second dimension
// (the loss state is sequential in time, so streams - not frames - are what runs side by side).
// d_in[i] / d_out[i]: uint16 [nframes][h][w] of stream i (HOST arrays of nstreams device pointers); low_errors / high_errors:
// HOST int[nstreams][nframes] or NULL (then nothing waits).
RIR_EXPORT int rir_lossy_step_multi_device(const int *handles, int nstreams, const unsigned short *const *d_in, unsigned short *const *d_out,
										   int nframes, int add_loss, int *low_errors, int *high_errors, void *stream)
{
	if (!device_ready())
		return -1;
	if (!handles || nstreams <= 0 || nstreams > 65535 || !d_in || !d_out || nframes <= 0)
	{
		log_error("rir_lossy_step_multi_device: invalid argument");
		return -1;
	}
	std::vector<std::shared_ptr<LossyObject>> os((size_t)nstreams);
	std::vector<LossyObject *> ptrs((size_t)nstreams);
	for (int i = 0; i < nstreams; ++i)
	{
		os[i] = lookup_as<LossyObject>(handles[i]);
		if (!os[i] || !d_in[i] || !d_out[i] || d_in[i] == d_out[i])
		{
			log_error("rir_lossy_step_multi_device: invalid handle or buffer");
			return -1;
		}
		if (frames_overlap("rir_lossy_step_multi_device", os[i]->st, d_in[i], d_out[i], nframes))
			return -1;
		for (int k = 0; k < i; ++k)
			if (os[k] == os[i])
			{
				log_error("rir_lossy_step_multi_device: a stream appears twice");
				return -1;
			}
		ptrs[i] = os[i].get();
		const LossyState &a = os[0]->st, &b = os[i]->st;
		if (a.w != b.w || a.h != b.h || a.hl != b.hl || a.frames != b.frames || os[i]->remove_bad_pixels)
		{
			log_error("rir_lossy_step_multi_device: the streams must share geometry and history length (and not repair bad pixels)");
			return -1;
		}
	}
	return lossy_step_streams(ptrs.data(), nstreams, d_in, d_out, nframes, add_loss, nullptr, low_errors, high_errors, (hipStream_t)stream);
}

// Which form stepped the groups of frames of the last run call this stream LED (a call of its own, or a multi-stream call it was first in):
// out[0] = groups offered to the constant-budget form (0: the call was not eligible - stdFactor != 0, frames stepped one by one, ...),
// out[1] = of those, groups it stepped (the others were declined on the device and stepped by the resident kernel).  Waits for `stream`.
RIR_EXPORT int rir_lossy_path_stats(int handle, int *out2, void *stream)
{
	auto o = lookup_as<LossyObject>(handle);
	if (!o || !out2)
	{
		log_error("rir_lossy_path_stats: invalid argument");
		return -1;
	}
	LossyRunScratch &sc = *o->scratch;
	out2[0] = sc.const_groups, out2[1] = 0;
	if (sc.const_groups > 0)
	{
		std::vector<unsigned int> w((size_t)sc.const_groups);
		if (!hip_ok(hipMemcpyAsync(w.data(), sc.const_ok.ptr, w.size() * 4, hipMemcpyDeviceToHost, (hipStream_t)stream), "D2H") ||
			!hip_ok(wait_stream((hipStream_t)stream), "sync"))
			return -1;
		for (unsigned int v : w)
			out2[1] += v != 0 ? 1 : 0;
	}
	return 0;
}

// The speculative form's books for the last run call this stream LED: out[0] = groups that went through its launches (0: the call was not
// eligible - stdFactor 0, frames stepped one by one, ...), out[1] = of those, groups that were offered (precondition held, no back-off),
// out[2] = groups it committed, out[3] = passes over all groups (a group's passes: the most any of its streams took).  Waits for `stream`.
RIR_EXPORT int rir_lossy_spec_stats(int handle, int *out4, void *stream)
{
	auto o = lookup_as<LossyObject>(handle);
	if (!o || !out4)
	{
		log_error("rir_lossy_spec_stats: invalid argument");
		return -1;
	}
	LossyRunScratch &sc = *o->scratch;
	out4[0] = sc.spec_groups, out4[1] = out4[2] = out4[3] = 0;
	if (sc.spec_groups > 0)
	{
		const size_t ng = (size_t)sc.spec_groups, ns = (size_t)sc.spec_streams;
		std::vector<unsigned int> w(ng * ns * 8), okw(ng);
		if (!hip_ok(hipMemcpyAsync(w.data(), sc.spec_ctl.ptr, w.size() * 4, hipMemcpyDeviceToHost, (hipStream_t)stream), "D2H") ||
			!hip_ok(hipMemcpyAsync(okw.data(), sc.const_ok.ptr, okw.size() * 4, hipMemcpyDeviceToHost, (hipStream_t)stream), "D2H") ||
			!hip_ok(wait_stream((hipStream_t)stream), "sync"))
			return -1;
		for (size_t g = 0; g < ng; ++g)
		{
			unsigned int passes = 0;
			for (size_t i = 0; i < ns; ++i)
				passes = std::max(passes, w[(g * ns + i) * 8 + 1]);
			out4[1] += w[g * ns * 8 + 4] != 0 ? 1 : 0;
			out4[2] += okw[g] != 0 ? 1 : 0;
			out4[3] += (int)passes;
		}
	}
	return 0;
}

// 0 when no run of frames this stream took part in has given up a wait between workgroups, -1 otherwise or on an invalid handle.
// Waits for the work queued on `stream` (calls queued on other streams are not covered).  The failure is sticky: the stream's state
// has been advanced by invalid frames, so from then on every status and every step of the stream - and of the streams that shared
// the failed call - returns -1 until it is destroyed.  Calls that return budgets check this themselves; queue-only calls do not.
RIR_EXPORT int rir_lossy_status(int handle, void *stream)
{
	auto o = lookup_as<LossyObject>(handle);
	if (!o)
	{
		log_error("rir_lossy_status: invalid handle");
		return -1;
	}
	hipStream_t st = (hipStream_t)stream;
	// the error word is with the leader of the last run call this stream took part in (itself, for a call of its own)
	LossyObject *l = o->leader();
	std::shared_ptr<Object> keep = o->lead.lock(); // (keeps a foreign leader alive while it is read)
	if (!l || !l->has_run())
		return hip_ok(wait_stream(st), "sync") && !o->is_failed() ? 0 : -1;
	unsigned int words[2]; // a wait that hit its clock / a launch that was called off because it did not become resident
	if (!l->queue_verdict_read(words, st) || !hip_ok(wait_stream(st), "sync"))
		return -1;
	l->checked(words[0] | words[1], st);
	if (o->is_failed())
	{
		log_error("rir_lossy_status: a run of frames gave up waiting (results invalid; the stream takes no more frames)");
		return -1;
	}
	return 0;
}

RIR_EXPORT void rir_lossy_destroy(int handle)
{
	if (lookup_as<LossyObject>(handle))
		remove_object(handle);
}
