// The bounded-loss stream (lossy_abi.cpp) as the saver sees it: one stream's state, its handle object and the step of a run of frames.
// Internal, C++ linkage.
#pragma once
#include <utility>

#include "lossy_kernels.h"
#include "runtime.h"

namespace rir
{
	// What a frame is stepped under: the variant (addLoss or the recording step, h264.cpp:2426 / :2253), bad-pixel repair, and the
	// parameters of H264_Saver::setParameter lowValueError / highValueError / stdFactor as they are when the frame comes.
	struct LossyParams
	{
		bool add_loss, remove_bad_pixels;
		int low, high;
		double std_factor;
	};

	// ---- bounded-loss step ---------------------------------------------------------------------
	// Host side of H264_Saver::addImageLossyNoCamera / addLoss (h264.cpp:2253-2424, :2426-2607): the
	// per-pixel work runs in lossy_kernels.hip; the error budget (40-frame window of the quirky
	// "stdDev" statistics, h264.cpp:2335-2385) is scalar double arithmetic done here from the exact
	// integer sums the GPU returns.
	struct LossyState
	{
		int w = 0, h = 0, hl = 0;
		int frames = 0;
		DeviceBuffer d_img, d_tmp, d_out, d_ref, d_prev, d_last, d_sums, d_cval, d_ccnt, d_ring, d_hist, d_stats, d_min, d_budget, d_decision, d_errs, d_tickets;
		LossyDeviceState dev{};
		DeviceBuffer d_shadow;	   // the speculative form of a run (lossy_kernels.h: LossySpec): where a pass leaves the state after the group
		LossyDeviceState shadow{}; // ... carved out of it (reserve_shadow)
		int bp_handle = 0;

		~LossyState();
		bool prepare(int w_, int h_, int hl_, int running_average, bool subtract_min);
		// img (host, full frame) -> d_out (device, full frame), copied to `out` (host) when it is not NULL.
		bool step(const unsigned short *img, unsigned short *out, const LossyParams &p, int &low_error, int &high_error);
		// pinned_img (PAGE-LOCKED host memory that stays untouched until the stream has passed this point) -> d_out (device),
		// queued without waiting; the frame's low / high error goes to d_errors (device int[2]).
		bool queue_host_frame(const unsigned short *pinned_img, const LossyParams &p, int *d_errors);
		// One frame, device to device (d_src and d_dst: full frames, distinct), queued on `st` without waiting: statistics,
		// error budget (lossy_budget_kernel) and update all run on the device.  d_errors: device int[2] that receives the
		// frame's low / high error (may be NULL).  Only the very first frame of a subtractMin stream waits (its minimum
		// becomes a parameter of every later launch).
		bool queue_frame(const uint16_t *d_src, uint16_t *d_dst, const LossyParams &p, int *d_errors, hipStream_t st);
		// what the kernels of the next frame need (the ring indices as they are now)
		LossyStep make_step(const uint16_t *tmp, const uint16_t *img, uint16_t *dst, const LossyParams &p, int *d_errors, int nstreams = 1);
		// the shadow arrays of the speculative form, allocated when a stream is first offered to it: as the state's own, ring included
		bool reserve_shadow();
		void advance_ring();
	};

	// The 256-byte header of the run kernel's exchange buffer (lossy_kernels.h: launch_lossy_run) holds the ticket in word 0, the error
	// word here, and the residency control block in words kLossyRunCtlWord .. + 3 (arrivals, decision, poison, epoch).
	constexpr int kLossyRunErrorWord = 16;

	struct LossyRunScratch; // the buffers of the run calls a stream leads, the exchange buffer among them (lossy_abi.cpp)

	// handle for the device-resident form of the bounded-loss step (rir_lossy_*)
	struct LossyObject : public Object
	{
		const char *type_name() const override { return "LossyStream"; }
		LossyState st;
		int low = 6, high = 2;
		double std_factor = 5;
		bool remove_bad_pixels = false;
		LossyParams params(bool add_loss) const { return LossyParams{add_loss, remove_bad_pixels, low, high, std_factor}; }
		std::unique_ptr<LossyRunScratch> scratch;
		// A resident run that gave up a wait has advanced the stream's state with invalid frames: the failure is STICKY - every
		// later step / status of a stream that took part in such a call fails until the stream is destroyed.  The error word lives
		// with the call's leading stream and says "some call since the last check"; so the leader numbers the calls it led and
		// keeps the ranges found invalid, and every member remembers who led its last run call and that call's number.
		bool failed = false;
		uint64_t led_calls = 0, led_clean = 0;				// as a leader: run calls led / of those, known good at the last check
		std::vector<std::pair<uint64_t, uint64_t>> led_bad; // calls in (first, second] are invalid
		std::weak_ptr<Object> lead;							// leader of the last run call this stream took part in, when that was another stream
		bool led_by_other = false;							// ... which `lead` then names (a leader that has been destroyed leaves no record)
		uint64_t lead_call = 0;								// that call's number with the leader (0: no run call yet)
		LossyObject();
		~LossyObject() override;
		LossyObject *leader();
		bool is_failed();
		bool has_run() const; // this stream has led a run call: there is an error word to read
		// Queues, on `st`, the read of the run kernel's error word (a wait between workgroups that hit its clock) into words[0] and of the
		// poison word (a launch that did not become resident and was called off, resident_device.h: its frames were not stepped) into
		// words[1]; `words` must stay put until the stream has passed this point.  Without a run call so far nothing is queued and the
		// words stay 0.  false: a copy could not be queued.
		bool queue_verdict_read(unsigned int *words, hipStream_t st);
		// files what a read of the error word (after a wait on the stream the calls were queued on) has shown
		void checked(unsigned int gave_up, hipStream_t st);
	};

	// The step of `nframes` frames for the streams os[0..nstreams) (checked by the callers: equal geometry and history length, no
	// bad-pixel repair).  d_errs: NULL, or per stream a DEVICE int[nframes][2] that receives the budgets (nothing is read back
	// then); otherwise low_errors / high_errors: HOST int[nstreams][nframes] or NULL.
	int lossy_step_streams(LossyObject *const *os, int nstreams, const unsigned short *const *d_in, unsigned short *const *d_out, int nframes, int add_loss,
						   int *const *d_errs, int *low_errors, int *high_errors, hipStream_t st, bool force_per_frame = false);
} // namespace rir
