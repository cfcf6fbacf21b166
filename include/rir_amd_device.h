/* librir_amd — device-resident batch entry points (extension of the librir C ABI).
 *
 * The reference ABI moves one frame per call through host pointers (reference
 * src/cpp/video_io/video_io.h:102,259 and src/cpp/signal_processing/signal_processing.h:29-88).
 * These entry points are the same operations on batches that already live in HBM, laid out
 * [n][h][w] row-major, asynchronous on a caller-supplied HIP stream (`stream` is a hipStream_t
 * passed as void*; NULL = HIP's null stream).  The per-frame reference entry points in
 * rir_amd_signal_processing.h / rir_amd_video_io.h are thin wrappers over these.
 *
 * All functions return 0 on success and -1 on error (reason via get_last_log_error) unless
 * stated otherwise.  No function falls back to the CPU: without a HIP device they fail.
 */
#ifndef RIR_AMD_DEVICE_H
#define RIR_AMD_DEVICE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C"
{
#endif

	/* 1 when a HIP device is visible, else 0 (never logs). */
	int rir_device_available(void);
	int rir_stream_synchronize(void *stream);

	/* The sizing rules of kernels whose workgroups wait for each other inside a launch ("resident launches", librir_amd/csrc/runtime.h),
	 * as plain host functions (no device needed; what the CPU tests check): workgroups of a kernel with blocks_per_cu resident
	 * workgroups per CU that one launch may hold on a device of `cus` CUs in `xcds` XCDs; and how `units` independent units (streams,
	 * sequences) of wgs_per_unit workgroups go through a kernel of that capacity: out2[0] = units per launch (0: a unit does not fit - the
	 * launch-per-frame / launch-per-iteration kernels are used), out2[1] = launches. */
	int rir_resident_capacity_rule(int blocks_per_cu, int cus, int xcds);
	int rir_resident_plan(int capacity, int wgs_per_unit, int units, int *out2);
	int rir_resident_plan_two_forms(int capacity_a, int capacity_b, int wgs_per_unit, int units, int *out3); /* a kernel in two forms: [2] = 1 when the larger, slower one saves a launch */

	/* ---- block codec (format RIRB1) ----------------------------------------------------------
	 * Replaces, for device-resident batches, the encode/decode the reference delegates to
	 * libx264 (reference src/cpp/video_io/h264.cpp:1022-1131 AddFrame, :3096-3229 GetFrame).
	 * A batch of nframes frames is cut in chunks of `gop` frames (key frame first, reference
	 * cadence h264.cpp:1052-1064); chunks and 512-pixel tiles are independent units. */
	typedef struct rir_codec_layout
	{
		int width, height, nframes, gop;
		int ntiles;				  /* ceil(width*height / 512) */
		int nchunks;			  /* ceil(nframes / gop) */
		int64_t hdr_bytes;		  /* uint64 [nchunks][ntiles][gop]   record headers (widths|mode|base) */
		int64_t tile_off_bytes;	  /* uint32 [nchunks][ntiles+1]      first word of a tile segment */
		int64_t chunk_off_bytes;  /* uint64 [nchunks+1]              first word of a chunk; last = total */
		int64_t stream_max_bytes; /* worst-case size of the compact stream */
		int64_t workspace_bytes;  /* scratch needed by rir_codec_encode_device */
	} rir_codec_layout;

	int rir_codec_layout_query(int width, int height, int nframes, int gop, rir_codec_layout *out);

	/* d_frames: uint16 [nframes][height][width].  Outputs sized per rir_codec_layout. */
	int rir_codec_encode_device(const unsigned short *d_frames, int width, int height, int nframes, int gop, unsigned long long *d_hdr,
								unsigned int *d_tile_off, unsigned long long *d_chunk_off, unsigned long long *d_stream, void *d_workspace,
								long long workspace_bytes, void *stream);

	/* The two stages of rir_codec_encode_device, callable separately (same workspace): stage 1 is
	 * the single pass over the raw frames (headers + sparse payload), stage 2 computes the
	 * offsets and gathers the payload into the dense stream. */
	int rir_codec_encode_tiles_device(const unsigned short *d_frames, int width, int height, int nframes, int gop, unsigned long long *d_hdr,
									  void *d_workspace, long long workspace_bytes, void *stream);
	int rir_codec_encode_compact_device(int width, int height, int nframes, int gop, unsigned int *d_tile_off, unsigned long long *d_chunk_off,
										unsigned long long *d_stream, void *d_workspace, long long workspace_bytes, void *stream);

	/* The SLOTTED form of an encoded batch: what stage 1 (rir_codec_encode_tiles_device) leaves - record headers in d_hdr, and in
	 * the workspace one length per (chunk, tile) segment plus every segment's payload at the start of a slot of slot_words
	 * 64-bit words whose place, slot index = chunk * ntiles + tile, depends on no length.  It is a complete encoded batch: the
	 * same records as the dense form, located by position instead of by the offsets of stage 2 (which exists to make the
	 * dense FILE form: chunk independence h264.cpp:1052-1064; offset-table precedent ZFile.cpp:434-447).  A consumer on the
	 * same device decodes it as it is - encode + decode then move 4WH + 2C bytes, the algorithmic minimum, in two launches. */
	typedef struct rir_codec_slots
	{
		int64_t slots_offset_bytes;		/* first slot, from d_workspace */
		int64_t slot_words;				/* distance of two slots, 64-bit words */
		int64_t seg_words_offset_bytes; /* uint32 [nchunks][ntiles] segment lengths in words, from d_workspace */
		int64_t nslots;					/* nchunks * ntiles */
	} rir_codec_slots;
	int rir_codec_slots_query(int width, int height, int nframes, int gop, rir_codec_slots *out);
	int rir_codec_decode_slots_device(const unsigned long long *d_hdr, const void *d_workspace, long long workspace_bytes, int width, int height,
									  int nframes, int gop, unsigned short *d_frames, int *d_error, void *stream);

	/* An encoder workspace (workspace_bytes of rir_codec_layout) allocated BY THE LIBRARY where the packing kernel runs fast for
	 * THIS frames buffer.  On MI355X device allocations fall into a few placement classes and the kernel, which reads the frames
	 * and writes the slots at the same pace, takes 10 % longer when both live in allocations of one class (DESIGN.md §7,
	 * profiles/r03_placement/README.md); nothing but a timing tells the class, so this call allocates up to max_tries further
	 * candidates, spacing_bytes apart (0: back to back), times stage 1 on each with HIP events and keeps the first one that is
	 * 7 % faster than the first, else the fastest; everything else it allocated is freed before it returns.  times_us: HOST
	 * float[max_tries + 1] or NULL (the kept candidate's time first), *ntimes = entries filled.  One-off set-up, a few ms. */
	int rir_codec_workspace_create_device(const unsigned short *d_frames, int width, int height, int nframes, int gop, int max_tries,
										  long long spacing_bytes, void **d_workspace, float *times_us, int *ntimes, void *stream);
	void rir_codec_workspace_destroy_device(void *d_workspace);

	/* The same placement for ANY pair of buffers that a kernel walks at the same pace - the input and the output of the frame-buffer
	 * kernels (translate, gaussian_filter, the fused chain, the 3x3 median: 5-10 % between the classes): `bytes` of device memory in another
	 * placement class than d_other, found by timing a plain streaming copy from d_other into each candidate.  Arguments as for
	 * rir_codec_workspace_create_device; release with rir_buffer_destroy_device. */
	int rir_buffer_create_beside_device(const void *d_other, long long other_bytes, long long bytes, int max_tries, long long spacing_bytes,
										void **d_buffer, float *times_us, int *ntimes, void *stream);
	void rir_buffer_destroy_device(void *d_buffer);

	/* The encode as one kernel that writes the dense stream directly (segments staged in LDS, decoupled look-back): same
	 * outputs bit for bit, fewer bytes through HBM, not faster on MI355X.  rir_codec_encode_status (waits for the
	 * stream): 0 = the last single-pass encode on this workspace completed, 1 = a look-back gave up, the stream is incomplete. */
	int rir_codec_encode_single_pass_device(const unsigned short *d_frames, int width, int height, int nframes, int gop, unsigned long long *d_hdr,
											unsigned int *d_tile_off, unsigned long long *d_chunk_off, unsigned long long *d_stream,
											void *d_workspace, long long workspace_bytes, void *stream);
	int rir_codec_encode_status(const void *d_workspace, void *stream);

	/* The PACKED form of an encoded batch: the dense stream without the order.  One pass over the frames (one kernel), and
	 * the encoded batch occupies exactly its payload + tables - what can be kept, sent between devices or written:
	 *   d_hdr        uint64 [nchunks][ntiles][gop]  record headers, as in every form
	 *   d_seg_pos    uint64 [nchunks][ntiles]       first 64-bit word of segment (chunk, tile) in d_stream
	 *   d_seg_words  uint32 [nchunks][ntiles]       its length in words
	 *   d_stream     two extents without holes, [0, low) and [capacity - high, capacity): the segments back to back in ORDER OF
	 *                ARRIVAL (the order differs from run to run, every segment's words are the canonical ones) - a table of
	 *                positions instead of an order, as the reference's own ZFile container keeps for its records (ZFile.cpp:434-447)
	 * A segment is staged in LDS and, when its length is known, handed the next free words by one atomic add: no second pass
	 * (rir_codec_encode_compact_device), no look-back (rir_codec_encode_single_pass_device), no worst-case slots (the slotted form).
	 * Two cursors because one is a bottleneck (12 800 returning adds on one address: 16 ns each), from the two ENDS of the
	 * capacity so that they share it.  stream_capacity_words is what the caller provides at d_stream - a budget, not a worst case
	 * (stream_budget_bytes = 8 bits per pixel; the reference documents a factor of about 5, docs/video_io.md:13): a batch that
	 * needs more is not written beyond it, the status says so and how many words it needs.  The workspace holds the control
	 * block and an arena for what does not fit a wave's LDS staging (noisy data only): workspace_min_bytes always works for
	 * data within the budget, workspace_max_bytes for any data.
	 * rir_codec_encode_packed_status (waits for the stream): out[0] = low, out[1] = high (words; the batch needs low + high),
	 * out[2] = arena words asked for; returns 0 = complete, 1 = stream capacity exceeded, 2 = arena exceeded (3 = both), -1 = error.
	 * Decoding checks every segment against stream_words before it reads through it. */
	typedef struct rir_codec_packed_layout
	{
		int ntiles, nchunks;
		int64_t hdr_bytes, seg_pos_bytes, seg_words_bytes;
		int64_t stream_budget_bytes; /* 8 bits per pixel: half the raw size */
		int64_t stream_max_bytes;	 /* any data fits */
		int64_t workspace_min_bytes, workspace_max_bytes;
	} rir_codec_packed_layout;
	int rir_codec_packed_query(int width, int height, int nframes, int gop, rir_codec_packed_layout *out);
	int rir_codec_encode_packed_device(const unsigned short *d_frames, int width, int height, int nframes, int gop, unsigned long long *d_hdr,
									   unsigned long long *d_seg_pos, unsigned int *d_seg_words, unsigned long long *d_stream,
									   long long stream_capacity_words, void *d_workspace, long long workspace_bytes, void *stream);
	int rir_codec_encode_packed_status(const void *d_workspace, unsigned long long *out3, void *stream);
	/* rir_codec_encode_packed_device in its two halves (the reset of the workspace's control block is a fill launch of its own).  _launch_
	 * packs into a workspace whose control block is zero: just reset on the same stream, or left so by the packed encode before it on that
	 * stream - a launch that runs to its end zeroes the block again and leaves its result for rir_codec_encode_packed_status, so a caller
	 * that knows its workspace is clean encodes with one launch. */
	int rir_codec_packed_reset_device(void *d_workspace, long long workspace_bytes, void *stream);
	int rir_codec_encode_packed_launch_device(const unsigned short *d_frames, int width, int height, int nframes, int gop, unsigned long long *d_hdr,
											  unsigned long long *d_seg_pos, unsigned int *d_seg_words, unsigned long long *d_stream,
											  long long stream_capacity_words, void *d_workspace, long long workspace_bytes, void *stream);
	int rir_codec_decode_packed_device(const unsigned long long *d_hdr, const unsigned long long *d_seg_pos, const unsigned int *d_seg_words,
									   const unsigned long long *d_stream, long long stream_words, int width, int height, int nframes, int gop,
									   unsigned short *d_frames, int *d_error, void *stream);

	/* *d_error (device int, zero it first) becomes 1 when a malformed table/record was met.  stream_words = number of
	 * 64-bit words readable at d_stream: the tables are untrusted (they may come from a file) and a (chunk, tile)
	 * segment that does not lie inside [0, stream_words) is rejected before anything is read through it. */
	int rir_codec_decode_device(const unsigned long long *d_hdr, const unsigned int *d_tile_off, const unsigned long long *d_chunk_off,
								const unsigned long long *d_stream, long long stream_words, int width, int height, int nframes, int gop,
								unsigned short *d_frames, int *d_error, void *stream);

	/* Decode of chunks that do not form one contiguous batch - chunks gathered from several shards (the exchange step of
	 * the multi-GPU path, reference chunk independence h264.cpp:1052-1064), or a selection of a file's chunks.  Entry k of
	 * the tables is one chunk (hdr[k][ntiles][gop], tile_off[k][ntiles+1], chunk_off[k..k+1]); d_chunk_frames[2k] /
	 * [2k+1] = first frame / frame count (<= gop, 0 = skip) of that chunk inside d_frames (frames_capacity frames). */
	int rir_codec_decode_chunks_device(const unsigned long long *d_hdr, const unsigned int *d_tile_off, const unsigned long long *d_chunk_off,
									   const unsigned long long *d_stream, long long stream_words, int width, int height, int nchunks, int gop,
									   const long long *d_chunk_frames, long long frames_capacity, unsigned short *d_frames, int *d_error,
									   void *stream);

	/* gaussian_filter as the 2-D sum in the reference's own order (signal_processing.cpp:101-148: dx outer, dy inner, a rounding per product
	 * and per sum) instead of the separable form: results bit-identical to the reference's instead of within 2e-6 of them, in gaussian_filter,
	 * rir_gaussian_filter*_device and rir_filter_chain_device (which then runs its three steps one after the other on the device), at about
	 * three times the time.  Process-wide, default off; also RIR_GAUSSIAN_REFERENCE_ORDER=1 in the environment. */
	void rir_set_gaussian_reference_order(int on);
	int rir_gaussian_reference_order(void);

	/* ---- frame-buffer kernels -------------------------------------------------------------------
	 * translate: reference signal_processing.h:29 / Filters.h:249-326.  `type` is the numpy
	 * dtype char ('?','b','B','h','H','i','I','l','L','f','d'); d_offsets holds float (dx,dy)
	 * pairs - one pair per frame when per_frame_offsets != 0, else a single pair; background
	 * is a HOST pointer to one element; d_dst must be pre-filled by the caller (strategy
	 * "noborder" leaves border pixels as they are).  The extra strategy "noborder_source" gives the result of
	 * "noborder" on a destination pre-filled with a copy of the input - what the Python wrappers do
	 * (rir_signal_processing.py:54-55) - without that copy: d_dst need not be initialised. */
	int rir_translate_device(int type, const void *d_src, void *d_dst, int w, int h, int nframes, const float *d_offsets, int per_frame_offsets,
							 const void *background, const char *strategy, void *stream);

	/* gaussian_filter: reference signal_processing.h:33 / signal_processing.cpp:79-148. */
	int rir_gaussian_filter_device(const float *d_src, float *d_dst, int w, int h, int nframes, float sigma, void *stream);

	/* The same two filters with the dtype conversions the Python callers do around them folded in (no
	 * converted copy of the frames in memory): gaussian_filter(img.astype(float32)) for uint16 frames
	 * (sigma < 2.5), and translate(float32 img, ...).astype(uint16) - the value is rounded to float first,
	 * then truncated, exactly as the two-step form.  background: HOST pointer to one uint16. */
	int rir_gaussian_filter_u16_device(const unsigned short *d_src, float *d_dst, int w, int h, int nframes, float sigma, void *stream);
	int rir_translate_f32_u16_device(const float *d_src, unsigned short *d_dst, int w, int h, int nframes, const float *d_offsets,
									 int per_frame_offsets, const void *background, const char *strategy, void *stream);

	/* The filter chain callers run before recording (reference tests/python/test_rir.py and BASELINE configs[2]:
	 * BadPixels.correct (BadPixels.cpp:34-66) -> gaussian_filter (signal_processing.cpp:101-148) -> translate
	 * (Filters.h:249-326) -> astype(uint16)) fused into ONE pass over the frames: 4 bytes of HBM traffic per pixel
	 * instead of 14.  Output bit-identical to rir_bad_pixels_correct_device + rir_gaussian_filter_u16_device +
	 * rir_translate_f32_u16_device.  bad_pixels_handle: from rir_bad_pixels_create_device, or 0 to skip that stage.
	 * strategy "nearest" or "background"/"constant" (background: HOST pointer to one uint16); sigma < 2.5;
	 * d_src != d_dst; offsets as for rir_translate_device.  The repair table lives in the bad-pixels object: one call at a
	 * time per handle. */
	int rir_filter_chain_device(int bad_pixels_handle, const unsigned short *d_src, unsigned short *d_dst, int w, int h, int nframes, float sigma,
								const float *d_offsets, int per_frame_offsets, const void *background, const char *strategy, void *stream);

	/* find_median_pixel[_mask]: reference signal_processing.h:39-44 / Filters.cpp:56-101.
	 * d_result: int32[nframes]; d_hist: unused, may be NULL (the counting happens in LDS); d_mask may be NULL. */
	int rir_find_median_pixel_device(const unsigned short *d_img, const unsigned char *d_mask, int size, int nframes, float percent, int *d_result,
									 unsigned int *d_hist, void *stream);

	/* bad pixels: reference signal_processing.h:80-88 / BadPixels.cpp:13-66.  The handle returned
	 * by the *_create_* functions is in the same int namespace as every other librir object and
	 * is released with bad_pixels_destroy().  Returns 0 on error. */
	int rir_bad_pixels_create_device(const unsigned short *d_first_image, int width, int height, void *stream);
	int rir_bad_pixels_correct_device(int handle, const unsigned short *d_in, unsigned short *d_out, int nframes, void *stream);
	int rir_bad_pixels_info(int handle, int *info3, int *xy, int cap);

	/* read-back path of the loader: reference IRFileLoader.cpp:693-716 (detector on the first
	 * `rows` rows), :722-802 (in-place repair), :617-627 (motion removal, d_shifts = (x,y) float
	 * pairs per frame; d_dst != d_src). */
	int rir_bad_pixels_create_rows_device(const unsigned short *d_first_image, int width, int height, int rows, void *stream);
	int rir_remove_bad_pixels_device(int handle, unsigned short *d_img, int rows, int nframes, void *stream);
	int rir_remove_motion_device(const unsigned short *d_src, unsigned short *d_dst, int w, int h, int rows, int nframes, const float *d_shifts,
								 void *stream);

	/* 3x3 median filter: reference Filters.h:71-129 (template without C export upstream). */
	int rir_median_filter_device(const unsigned short *d_src, unsigned short *d_dst, int w, int h, int nframes, void *stream);

	/* Temporal median of a uint16 stack d_src[nframes][h][w] (extension).  Output k < count is frame t = first + k * step: with
	 * r = window / 2 (window odd, 1..63), S = frames max(0, t - r) .. min(nframes - 1, t + r) - truncated at the ends of THIS stack, never
	 * padded - and m = sorted(S)[|S| / 2] (the upper median when |S| is even), d_dst[k] = m where |src[t] - m| > threshold (0..65535;
	 * 0 gives the plain median), src[t] elsewhere; rows y >= `rows` (0..h) are copied unchanged.  A caller that passes a batch with r frames
	 * of halo on either side gets the bits of one call over the whole sequence.  Asynchronous on `stream`; d_dst holds `count` frames and
	 * may not overlap d_src.  count 0: nothing is done.  0 / -1 (invalid argument, overlap, no device). */
	int rir_temporal_median_device(const unsigned short *d_src, unsigned short *d_dst, int w, int h, int nframes, int first, int count, int step,
								   int window, int threshold, int rows, void *stream);

	/* Flat morphology of a stack d_src[nframes][h][w] into d_dst (same type and shape; extension).  type: 'H' uint16, 'B' uint8, '?' bool
	 * (one byte, 0 / 1).  The structuring element is a centred rectangle size_y x size_x, both odd, 1..15.  The image is the first `rows`
	 * (0..h) rows of a frame: rows y >= `rows` are copied unchanged and no window reads them.  With W(y, x) the window around (y, x)
	 * CLIPPED to the image (truncated, never padded), E(f)(y, x) = min of f over W(y, x), D(f)(y, x) = max of f over W(y, x), and
	 *   op 0 erode E(f)   1 dilate D(f)   2 open D(E(f))   3 close E(D(f))   4 tophat f - D(E(f))   5 blackhat E(D(f)) - f
	 *   6 gradient D(f) - E(f)
	 * each stage of open / close with its own clipped windows (the second stage never sees a first-stage value outside the image); the
	 * three differences are never negative.  Per frame this is scipy.ndimage.minimum_filter / maximum_filter(size=(size_y, size_x),
	 * mode="nearest") composed stage by stage.  Size 1 x 1: ops 0-3 copy, ops 4-6 give zeros; a window larger than the image clips.
	 * One launch that reads the stack once and writes it once, whatever the op and the size: there is no workspace.  Asynchronous on
	 * `stream`; d_dst may not overlap d_src.  nframes 0: nothing is done, 0.  -1 with the reason logged (argument errors before the device
	 * is looked for): unknown type or op, an even size or one outside 1..15, rows outside 0..h, w or h < 1, nframes < 0, a null pointer,
	 * overlap, no device. */
	int rir_morphology_device(int type, const void *d_src, void *d_dst, int w, int h, int nframes, int op, int size_x, int size_y, int rows, void *stream);

	/* Spatial rank filter of a stack d_src[nframes][h][w] into d_dst (same type and shape; extension).  type: 'H' uint16, 'B' uint8, '?' bool
	 * (one byte, 0 / 1).  The window is a centred rectangle size_y x size_x, both odd, 1..15; 0 <= rank < size_x * size_y.  The image is
	 * the first `rows` (0..h) rows of a frame: rows y >= `rows` are copied unchanged and no window reads them.  For y < rows,
	 *   d_dst[n][y][x] = the element of 0-based rank `rank` (in ascending order) among the size_y * size_x values
	 *                    d_src[n][clamp(y + dy, 0, rows - 1)][clamp(x + dx, 0, w - 1)],  |dy| <= size_y / 2, |dx| <= size_x / 2:
	 * the window is always FULL, with coordinates replicated at the border; it is not clipped.  Per frame this is
	 * scipy.ndimage.rank_filter(frame[:rows], rank, size=(size_y, size_x), mode="nearest"); rank size_x * size_y / 2 is scipy's
	 * median_filter, rank 0 and rank size_x * size_y - 1 are op 0 and op 1 of rir_morphology_device (a replicated pixel changes no min or
	 * max).  This is NOT rir_median_filter_device at 3 x 3: that one takes the median of 3 along an edge and the min of 2 in a corner.
	 * All integer, bit for bit.  One launch that reads the stack once and writes it once: there is no workspace.  Asynchronous on
	 * `stream`; d_dst may not overlap d_src.  nframes 0: nothing is done, 0.  -1 with the reason logged (argument errors before the device
	 * is looked for): unknown type, an even size or one outside 1..15, rank outside 0 .. size_x * size_y - 1, rows outside 0..h, w or
	 * h < 1, nframes < 0, a null pointer, overlap, no device. */
	int rir_rank_filter_device(int type, const void *d_src, void *d_dst, int w, int h, int nframes, int rank, int size_x, int size_y, int rows,
							   void *stream);

	/* Local window statistics of a stack d_src[nframes][h][w] (extension).  type: 'H' uint16, 'B' uint8, '?' bool (one byte, 0 / 1).  The
	 * window is a centred rectangle size_y x size_x, both odd, 1..15, of n = size_x * size_y cells, always FULL with coordinates replicated
	 * at the border as in rir_rank_filter_device; the image is the first `rows` (0..h) rows of a frame and no window reads the others.
	 * With v(dy, dx) = d_src[n][clamp(y + dy, 0, rows - 1)][clamp(x + dx, 0, w - 1)], |dy| <= size_y / 2, |dx| <= size_x / 2, for y < rows
	 *   d_sum[n][y][x]   = S = the sum of the v(dy, dx)            (int32; at most 225 * 65535 = 14 745 375)
	 *   d_sumsq[n][y][x] = Q = the sum of the v(dy, dx)^2          (int64; at most 225 * 65535^2 = 966 338 150 625)
	 *   d_mean[n][y][x]  = (S + n / 2) / n in integer division     (the type of d_src; the mean rounded half up)
	 * and in rows y >= `rows` the two sums are 0 and d_mean is a copy of d_src.  Each output may be null - it is then not computed -, at
	 * least one must not be.  n Q - S^2 is n^2 times the window's population variance, in exact integers.  All integer, bit for bit.  One
	 * launch per 65535 frames that reads the stack once and writes each output once: no workspace.  Asynchronous on `stream`; no output may
	 * overlap d_src or another output.  nframes 0: nothing is done, 0.  -1 with the reason logged (argument errors before the device is
	 * looked for): unknown type, an even size or one outside 1..15, rows outside 0..h, w or h < 1, nframes < 0, a null d_src, no output,
	 * overlap, no device. */
	int rir_local_stats_device(int type, const void *d_src, int w, int h, int nframes, int size_x, int size_y, int rows, int *d_sum, long long *d_sumsq,
							   void *d_mean, void *stream);

	/* The z-score mask of a stack d_src[nframes][h][w] (extension): d_mask[nframes][h][w], one byte 0 / 1 a pixel - what
	 * rir_label_images_device and rir_morphology_device take.  Types, window, border and rows as rir_local_stats_device.  With v the pixel,
	 * S and Q its window's sums, d = n v - S and V = n Q - S^2 (>= 0), k = k_num / k_den (0 <= k_num <= 255, 1 <= k_den <= 64), delta in
	 * -65535..65535 and polarity
	 *   0 above: d_mask = 1 where d > delta n and d^2 k_den^2 > k_num^2 V   (v - mean > delta and |v - mean| > k sigma, both strict, with
	 *                                                                        the exact rational mean and population sigma, centre included)
	 *   1 below: the same with -d in the first test                         2 both: above or below
	 * and 0 elsewhere and in rows y >= `rows`.  A constant window gives 0; k_num 0 is "off the local mean by more than delta".  The limits
	 * of the parameters keep every product inside int64; the test is exact.  One launch per 65535 frames that reads the stack once and
	 * writes the mask once (neither sum is stored): no workspace.  Asynchronous on `stream`; d_mask may not overlap d_src.  nframes 0:
	 * nothing is done, 0.  -1 with the reason logged (argument errors before the device is looked for): as rir_local_stats_device, and
	 * k_num, k_den, delta or polarity outside their ranges. */
	int rir_local_threshold_device(int type, const void *d_src, unsigned char *d_mask, int w, int h, int nframes, int size_x, int size_y, int rows,
								   int k_num, int k_den, int delta, int polarity, void *stream);

	/* Exact Euclidean distance transform of a stack of masks or label maps d_src[nframes][h][w] (extension): d_dist2[nframes][h][w], int32,
	 * the SQUARED distance of every pixel to the nearest background pixel of its frame, and - unless d_index is NULL - d_index[nframes][h][w],
	 * int32, which pixel that is.  type: '?' bool (one byte, 0 / 1), 'B' uint8, 'H' uint16, 'i' int32.  A cell is background when it equals
	 * `background` (which must lie in the type's range: 0..1, 0..255, 0..65535, any int), foreground otherwise.  The image is the first
	 * `rows` (0..h) rows of a frame; rows y >= `rows` are read by nothing and get dist2 0 and index y * w + x, their own.  For an image
	 * pixel p = (y, x):
	 *   dist2[p] = min over the background pixels q = (qy, qx) of the image of (y - qy)^2 + (x - qx)^2      (0 on background)
	 *   index[p] = the LOWEST flat index qy * w + qx among the background pixels at that minimum
	 * An image without a background pixel gets dist2 RIR_DIST2_NONE and index -1 everywhere.  border 1: everything outside the image
	 * counts as background too - dist2[p] = min(dist2[p], b^2), b = min(x + 1, w - x, y + 1, rows - y) - and index[p] = -1 where the
	 * outside is STRICTLY nearer than every background pixel.  1 <= w, h <= 16384, so every distance fits.  Where a background pixel
	 * exists, dist2 is round(scipy.ndimage.distance_transform_edt(src != background)^2); scipy's return_indices breaks ties differently.
	 * With fg = src != background and r2 = floor(r^2): fg & (dist2 > r2) is the erosion of fg by the Euclidean disc of radius r with
	 * the outside foreground (border 0) or background (border 1), and dist2 of the inverted mask <= r2 its dilation.  All integer, bit for
	 * bit, the same bits for any split of the stack into calls.  Two launches per group of frames, work per row and per column linear in
	 * its length, nothing on the host in between.  d_work: device memory, 8-byte aligned, at least ONE frame's share of
	 * rir_distance_transform_workspace_bytes(w, h, nframes, want_indices) (which is nframes shares, 256 MiB worth of them at most, or 0
	 * when w, h, nframes or want_indices are refused): the stack goes through in groups of as many frames as the workspace holds.
	 * Asynchronous on `stream`; no output or the workspace may overlap the input or another output.  nframes 0: nothing is done, 0.
	 * -1 with the reason logged (argument errors before the device is looked for): unknown type, background outside the type's range,
	 * border not 0 / 1, rows outside 0..h, w or h outside 1..16384, nframes < 0, a null d_src, d_dist2 or d_work, overlap, a workspace
	 * that is too small or misaligned, no device. */
#define RIR_DIST2_NONE 0x7fffffff
	size_t rir_distance_transform_workspace_bytes(int w, int h, int nframes, int want_indices);
	int rir_distance_transform_device(int type, const void *d_src, int w, int h, int nframes, int background, int border, int rows, int *d_dist2,
									  int *d_index /* may be NULL */, void *d_work, size_t work_bytes, void *stream);

	/* Grey-level morphological reconstruction of a marker under a mask (extension): d_dst[nframes][h][w] from the stack d_mask[nframes][h][w]
	 * and, in marker mode 0, the stack d_marker of the same type and shape.  type: 'H' uint16, 'B' uint8, '?' bool (one byte, 0 / 1), top =
	 * the type's maximum.  Per frame; the image is the first `rows` (0..h) rows of a frame, rows y >= `rows` of d_dst are a copy of the MASK
	 * and nothing reads them.  N(p) is p and its neighbours inside the image: the 3x3 window clipped to the image (connectivity 8) or the
	 * cross (connectivity 4); there is no padding.  With G the mask and F the marker:
	 *   method 0, reconstruction by dilation: F0 = min(F, G) (a marker above the mask is clamped, not refused), R the fixed point of
	 *     F_{k+1}(p) = min(G(p), max of F_k over N(p)).  Equivalently R(p) = the maximum, over every pixel q and every connected path from q
	 *     to p, of min(F0(q), min of G along the path) - which no order of evaluation enters.
	 *   method 1, reconstruction by erosion, the dual: F0 = max(F, G), F_{k+1}(p) = max(G(p), min of F_k over N(p)).
	 * marker_mode 0: F = d_marker.  1: F = G - param saturating at 0 (dilation), G + param saturating at top (erosion), param in 0..top; no
	 * marker stack is stored or read.  2: F = G on row 0, row rows - 1, column 0 and column w - 1, elsewhere 0 (dilation) or top (erosion).
	 * d_marker must be NULL unless the mode is 0.  output 0: R.  1: the difference, G - R (dilation) or R - G (erosion), never negative.
	 * So f - R(f - h, f) = (method 0, mode 1, param h, output 1) is the h-dome, which keeps what stands more than h above its surround
	 * whatever its extent, (method 1, mode 2, output 0) fills the holes and basins that do not reach the border, and (method 0, mode 2,
	 * output 1) removes what is connected to it.  All integer, bit for bit, the same bits for any split of the stack into calls or groups.
	 * Rounds of one launch each: a workgroup converges a tile of 64 x 32 pixels in LDS and raises its frame's flag when a pixel moved, in
	 * place over d_dst; the host reads the flags between rounds and stops after a round that wrote nothing - at most w * rows + 2 rounds,
	 * beyond which the call fails with "did not converge" (a correct kernel cannot get there).  The call is therefore SYNCHRONOUS with the
	 * host: it waits for `stream` (for nothing else), and cannot be captured into a graph.  *rounds (host memory, may be NULL): the rounds
	 * the call took, the largest number over its groups of frames.  d_work: device memory, 8-byte aligned, at least ONE frame's share of
	 * rir_reconstruct_workspace_bytes(type, w, h, nframes) (which is nframes shares, or 0 when its arguments are refused): the stack goes
	 * through in groups of as many frames as the workspace holds.  d_dst and the workspace may overlap neither input; d_marker == d_mask
	 * is allowed and gives the mask back.  nframes 0: nothing is done, 0.  -1 with the reason logged (argument errors before the device is
	 * looked for): unknown type, method, connectivity, marker mode or output, param outside 0..top, rows outside 0..h, w or h < 1 or
	 * w * h >= 2^31, nframes < 0, a null d_mask, d_dst or d_work, a marker with mode 1 or 2 or none with mode 0, overlap, a workspace that
	 * is too small or misaligned, no device. */
	size_t rir_reconstruct_workspace_bytes(int type, int w, int h, int nframes);
	int rir_reconstruct_device(int type, const void *d_mask, const void *d_marker, void *d_dst, int w, int h, int nframes, int method, int connectivity,
							   int marker_mode, int param, int output, int rows, void *d_work, size_t work_bytes, int *rounds, void *stream);

	/* Per-region statistics of a uint16 stack d_frames[nframes][h][w] (extension).  d_labels: int32, one map [h][w] for every frame
	 * (labels_per_frame 0) or one per frame [nframes][h][w] (1).  For frame f and region r < nregions (1..2^24), P = the flat indices
	 * i = y * w + x whose label is r; labels outside [0, nregions) are ignored.  Outputs [nframes][nregions]: d_count = |P|, d_sum and
	 * d_sumsq = the exact sums of the values and of their squares, d_min / d_max = the extremes over P, d_argmin / d_argmax = the lowest i
	 * in P that holds them; an empty region has count, sums 0 and -1 for the other four.  Bitwise reproducible.  d_work: device memory,
	 * 8-byte aligned, at least rir_region_stats_workspace_bytes(...) (0: arguments refused).  Asynchronous on `stream`; no output or
	 * the workspace may overlap an input or another output.  nframes 0: nothing is done.  0 / -1 (invalid argument, null pointer,
	 * overlap, workspace too small, no device). */
	int rir_region_stats_device(const unsigned short *d_frames, const int *d_labels, int w, int h, int nframes, int labels_per_frame, int nregions,
								int *d_count, long long *d_sum, long long *d_sumsq, int *d_min, int *d_max, int *d_argmin, int *d_argmax,
								void *d_work, size_t work_bytes, void *stream);
	size_t rir_region_stats_workspace_bytes(int w, int h, int nframes, int labels_per_frame, int nregions);

	/* Per-region geometry of int32 label maps (extension): where every region is and how it is spread, optionally weighted by a uint16
	 * stack d_frames[nframes][h][w].  d_labels, labels_per_frame, nregions (1..2^24) and the rule that labels outside [0, nregions) are
	 * ignored are those of rir_region_stats_device.  For frame f and region r, P = the pixels of f whose label is r, x = i % w, y = i / w
	 * for the flat index i, v = the pixel's value.  Outputs, [nframes][nregions] leading: d_count = |P| (int32); d_bbox[..][4] = xmin,
	 * ymin, xmax, ymax over P, inclusive (int32; -1, -1, -1, -1 for an empty region); d_moments[..][5] = the exact sums over P of x, y,
	 * x^2, x * y, y^2 (int64; zeros for an empty region); d_weighted[..][3] = the exact sums over P of v, v * x, v * y (int64), written
	 * only when frames are given: d_weighted is null exactly when d_frames is.  With d_frames null only the labels are read and nframes
	 * counts label maps: labels_per_frame 1, or nframes <= 1.  With frames and one shared map every frame still gets its own row of all
	 * outputs.  Bounds: w, h <= 32768 and w * h < 2^31; every sum is then below 2^62 (the largest is 65535 * 32767 * 2^31).  All
	 * combination is integer add, min and max: bitwise reproducible, whatever the launch geometry.  d_work: device memory, 8-byte aligned,
	 * at least rir_region_geometry_workspace_bytes(...) bytes (0: arguments refused; `weighted` 1 when frames will be given, else 0).
	 * Asynchronous on `stream`; no output or the workspace may overlap an input or another output.  nframes 0: nothing is done.  0 / -1
	 * (invalid argument, null pointer, overlap, workspace too small, no device). */
	int rir_region_geometry_device(const int *d_labels, const unsigned short *d_frames /* or null */, int w, int h, int nframes,
								   int labels_per_frame, int nregions, int *d_count, int *d_bbox, long long *d_moments,
								   long long *d_weighted /* null iff d_frames is null */, void *d_work, size_t work_bytes, void *stream);
	size_t rir_region_geometry_workspace_bytes(int w, int h, int nframes, int labels_per_frame, int nregions, int weighted);

	/* Per-region quantiles of a uint16 stack d_frames[nframes][h][w] (extension), frames and label maps as rir_region_stats_device takes
	 * them, nregions 1..65 536.  `percents`: HOST memory, npercents (1..8) floats in [0, 1].  For frame f, region r and percent p_j, V = the
	 * values of the pixels of f whose label is r, c = |V| and t = (int)roundf((float)c * p_j) - the product in float32, rounded half away
	 * from zero: the reference's masked rule (Filters.cpp:92).  d_count[f][r] = c; d_values[f][r][j] = -1 when c == 0 (find_median_pixel_mask
	 * gives 0 there; -1 is the empty region of rir_region_stats_device), 0 when t == 0 (so p = 0 gives 0, not the minimum), else the t-th
	 * smallest element s of V (1-based) when s < 65535, and 0 when s == 65535 or t > c (the reference counts into 65 535 bins: 65535 is
	 * in the population but in no bin; t > c needs a (float)c that rounds up).  For c > 0 that is find_median_pixel_mask(frame f,
	 * labels == r, p_j).  Integer arithmetic apart from t; bitwise reproducible.  d_work: device memory, 8-byte aligned, of at least
	 * B = nregions * (1040 + 1032 * npercents) bytes; the stack is worked through in groups of work_bytes / B frames, and every size gives
	 * the same bits.  rir_region_quantiles_workspace_bytes: B * min(max(nframes, 1), max(1, 256 MiB / B)), or 0 for refused arguments.
	 * Asynchronous on `stream` (`percents` is read before the call returns); no output or the workspace may overlap an input or another
	 * output.  nframes 0: nothing is done.  0 / -1 (invalid argument, null pointer, overlap, workspace too small, no device). */
	int rir_region_quantiles_device(const unsigned short *d_frames, const int *d_labels, int w, int h, int nframes, int labels_per_frame,
									int nregions, const float *percents /* HOST, npercents floats */, int npercents,
									int *d_count, int *d_values, void *d_work, size_t work_bytes, void *stream);
	size_t rir_region_quantiles_workspace_bytes(int w, int h, int nframes, int labels_per_frame, int nregions, int npercents);

	/* Per-region histograms of a uint16 stack d_frames[nframes][h][w] (extension), frames and label maps as rir_region_stats_device takes
	 * them (one map [h][w], or [nframes][h][w] with labels_per_frame 1; labels outside [0, nregions) are ignored), nregions 1..65 536.
	 * d_labels null: the whole image is region 0 - nregions must be 1 and labels_per_frame 0 - and only the frames are read, 2 bytes a
	 * pixel instead of 6.  Only the first `rows` (0..h) rows of every frame, and of every map, are counted; the frame stride stays w * h
	 * (the metadata rows of a WEST frame are left out as `rows` leaves them out of the filters).  Bins: nbins (1..65 536) bins of `width`
	 * (1..65 536) levels from `lo` (0..65 535), with nregions * nbins <= 2^24; lo + nbins * width may pass 65 536, the bins beyond stay 0.
	 * For frame f and region r, V = the values of the counted pixels of f whose label is r.  Outputs, all int32:
	 *   d_hist[f][r][b]     = the number of v in V with lo + b * width <= v < lo + (b + 1) * width,
	 *   d_outside[f][r][0]  = the number with v < lo,  d_outside[f][r][1] = the number with v >= lo + nbins * width,
	 *   d_count[f][r]       = |V|,  so that count == outside[0] + sum over b of hist + outside[1] always;
	 * an empty region has zeros everywhere.  d_count and d_outside may each be null: not wanted.  The device uses integer arithmetic only
	 * ((v - lo) / width is a shift for a power of two, else a multiply-high by a reciprocal computed on the host, exact for every 16-bit
	 * value) and every combination is a 32-bit integer add: bitwise reproducible, whatever the launch geometry.  The outputs are zeroed
	 * by the call and serve as the accumulators.  d_work: device memory, 8-byte aligned, at least rir_region_histogram_workspace_bytes(...)
	 * bytes - a small constant kept for uniformity with the other region entries; 0: arguments refused.  Asynchronous on `stream`; no
	 * output or the workspace may overlap an input or another output.  nframes 0: nothing is done, 0; rows 0: the outputs are zeroed, 0.
	 * 0 / -1 with the reason logged; a bad argument, a null pointer (other than d_labels, d_count, d_outside), a workspace too small and
	 * an overlap are refused before the device is looked for; then no device.  There is no CPU fallback. */
	int rir_region_histogram_device(const unsigned short *d_frames, const int *d_labels /* or null */, int w, int h, int rows, int nframes,
									int labels_per_frame, int nregions, int lo, int width, int nbins, int *d_count /* or null */, int *d_hist,
									int *d_outside /* or null */, void *d_work, size_t work_bytes, void *stream);
	size_t rir_region_histogram_workspace_bytes(int w, int h, int rows, int nframes, int labels_per_frame, int nregions, int nbins);

	/* Per-pixel statistics over time of a uint16 stack d_frames[nframes][h][w] (extension).  For pixel i = y * w + x, with v_f = d_frames[f][i],
	 * f = 0 .. nframes - 1, and a time origin t0 >= 0, the outputs [h][w] are: d_sum[i] = the exact sum of the v_f, d_sumsq[i] = the exact sum
	 * of their squares (int64), d_min[i] / d_max[i] = the extremes over f, d_argmin[i] / d_argmax[i] = t0 + f for the LOWEST f that holds the
	 * extreme (int32).  Two groups: the sums (d_sum, d_sumsq) and the extremes (d_min, d_max, d_argmin, d_argmax); the pointers of a group are
	 * all given or all null, and at least one group is given.  accumulate 0: the outputs are written from this stack alone.  accumulate 1: they
	 * are merged with what they hold, which must be the result of earlier calls over other time indices or the empty state (sums 0, -1 in
	 * the other four): sums add; the smaller minimum wins and, of equal minima, the lower time index; likewise for the maximum.  So any
	 * split of a sequence into batches, pushed in any order with the right t0, gives the bits of one call over the whole sequence.
	 * Bounds: w, h >= 1, w * h < 2^31, t0 + nframes <= 2^31 - 1; under them the int64 sums cannot overflow (65535^2 * 2^31 < 2^63).  No
	 * floating point is used on the device: the result is bitwise reproducible and independent of the order the workgroups run in.
	 * d_work: device memory, 8-byte aligned, at least rir_pixel_stats_workspace_bytes(w, h, nframes) bytes (0 only for refused arguments).
	 * Asynchronous on `stream`; no output or the workspace may overlap the input or another output.  nframes 0: 0, nothing is done.
	 * 0 / -1 (invalid argument, null or half-given group, overlap, workspace too small, no device). */
	int rir_pixel_stats_device(const unsigned short *d_frames, int w, int h, int nframes, int t0, int accumulate,
							   long long *d_sum, long long *d_sumsq, int *d_min, int *d_max, int *d_argmin, int *d_argmax,
							   void *d_work, size_t work_bytes, void *stream);
	size_t rir_pixel_stats_workspace_bytes(int w, int h, int nframes);

	/* Per-pixel quantiles over time of a uint16 stack d_frames[nframes][h][w] (extension): the rule of rir_region_quantiles_device applied
	 * to the time series of each pixel.  `percents`: HOST memory, npercents (1..8) floats in [0, 1].  For pixel i = y * w + x and percent
	 * p_j, V = the nframes values d_frames[f][i], c = nframes and t = (int)roundf((float)c * p_j) - the product in float32, rounded half
	 * away from zero.  d_values[j][y][x] (int32 [npercents][h][w], one image per percent) = -1 when c == 0, 0 when t == 0 or t > c, else the
	 * t-th smallest element s of V (1-based) when s < 65535, and 0 when s == 65535.  For c > 0 that is find_median_pixel(series of pixel i,
	 * p_j, mask of ones), and rir_region_quantiles_device over the stack viewed as one nframes x (h * w) image labelled by column.
	 * Bounds: w, h >= 1, w * h < 2^31, frames in all <= 2^31 - 1.  Integer arithmetic apart from t; bitwise reproducible, independent of the
	 * order the workgroups run in, of how a sequence is split into pushes and of the order of the pushes within a pass.
	 *
	 * The method is a radix select, P = rir_pixel_quantiles_passes() passes over the frames.  One call over a resident stack:
	 * rir_pixel_quantiles_device, with d_work device memory, 8-byte aligned, of at least rir_pixel_quantiles_workspace_bytes(w, h, nframes,
	 * npercents) = rir_pixel_quantiles_state_bytes(w, h, npercents) bytes (never 0 for valid arguments); nframes 0 fills d_values with -1.
	 *
	 * A sequence that is not resident is streamed P times.  The device state is opaque, rir_pixel_quantiles_state_bytes(w, h, npercents)
	 * = 72 * npercents * w * h bytes (0: arguments refused), 8-byte aligned; the ALL-ZERO state is the empty state, which the caller makes
	 * with a memset on the stream before the first push.  The host keeps the pass number and the frame count.  For pass = 0 .. P - 1:
	 * rir_pixel_quantiles_push_device for every batch of the sequence, in any order (nframes 0: nothing is done), then
	 * rir_pixel_quantiles_resolve_device once, with the same percents every time and total_frames = the frames of the whole sequence, the
	 * same in every pass.  The resolve of pass P - 1 writes d_values (null is accepted before); with total_frames 0 it fills them with -1.
	 * Every pass must see the same frames; the counts of states kept on several devices over parts of a sequence simply add.
	 *
	 * All calls are asynchronous on `stream`; `percents` is read before the call returns.  The values, the state or workspace and the
	 * frames may not overlap.  0 / -1 (invalid argument, null pointer, overlap, workspace or state too small, pass out of range, no
	 * device). */
	int    rir_pixel_quantiles_passes(void);
	size_t rir_pixel_quantiles_state_bytes(int w, int h, int npercents);
	size_t rir_pixel_quantiles_workspace_bytes(int w, int h, int nframes, int npercents);
	int    rir_pixel_quantiles_device(const unsigned short *d_frames, int w, int h, int nframes,
									  const float *percents /* HOST */, int npercents, int *d_values /* [npercents][h][w] */,
									  void *d_work, size_t work_bytes, void *stream);
	int    rir_pixel_quantiles_push_device(const unsigned short *d_frames, int w, int h, int nframes, int npercents, int pass,
										   void *d_state, size_t state_bytes, void *stream);
	int    rir_pixel_quantiles_resolve_device(int w, int h, const float *percents /* HOST */, int npercents, int pass,
											  long long total_frames, void *d_state, size_t state_bytes,
											  int *d_values /* written when pass == P - 1, may be null before */, void *stream);

	/* Connected components tracked through time (extension).  d_labels: int32 label maps [nframes][h][w] as rir_label_images_device writes
	 * them; d_counts: int[nframes], components + 1 per frame as it returns them, or null; nlabels = K >= 1.  Component k of frame t exists
	 * when 1 <= k < min(K, d_counts[t]) (1 <= k < K without d_counts); every other label value is background.  Components (t, a) and
	 * (t + 1, b) are linked when a pixel p has d_labels[t][p] == a and d_labels[t + 1][p] == b; a track is a connected set of components
	 * under these links; the node of (t, k) has index t * K + k, and tracks are numbered 1, 2, ... in the order of their lowest node
	 * (track 0 = background).  For a boolean stack labelled frame by frame this is the 3-D labelling with 4-connectivity inside a frame and
	 * the same pixel in adjacent frames, numbered in raster order of each component's first voxel.
	 * Outputs: d_track_of int[nframes][K], the track of each component, 0 where it does not exist; d_info int[2] = {tracks + 1, frames with
	 * d_counts[t] > K, whose components >= K were dropped}; tables of `table_entries` ints per track: d_first_frame, d_last_frame,
	 * d_first_label (the label of the lowest node, in frame first_frame) and d_components (nodes of the track) - entry 0 is -1, -1, 0, 0,
	 * entries from d_info[0] on are 0, tracks >= table_entries are not written; d_dst (or null) int32 [nframes][h][w], the track map
	 * d_track_of[t][d_labels[t][p]], 0 on the background, which may be d_labels itself.  Integer work, bitwise reproducible.  nframes 0:
	 * d_info = {1, 0} and the empty tables.  Bounds: w * h <= 0x7FFF0000, nframes * K <= 0x7FFF0000, table_entries >= 1.
	 * d_work: device memory, 8-byte aligned, at least rir_track_components_workspace_bytes(...) (0: arguments refused).  Asynchronous on
	 * `stream`; no output or the workspace may overlap an input or another output, except d_dst == d_labels.  0 / -1 (invalid argument,
	 * null pointer, overlap, workspace too small, no device). */
	int rir_track_components_device(const int *d_labels, const int *d_counts, int w, int h, int nframes, int nlabels, int *d_track_of, int *d_info,
									int *d_first_frame, int *d_last_frame, int *d_first_label, int *d_components, int table_entries, int *d_dst,
									void *d_work, size_t work_bytes, void *stream);
	size_t rir_track_components_workspace_bytes(int w, int h, int nframes, int nlabels);

	/* Polygon regions of interest rasterised into int32 label maps d_dst[nmaps][h][w], as rir_region_stats_device takes them (extension).
	 * d_xy: double [nsets][npoly][max_pts][2], the (x, y) vertices; d_npts: int [nsets][npoly], the vertices of each polygon (0..max_pts;
	 * any other count draws nothing); nsets = 1 (sets_per_map 0: one set for every map) or nmaps (1: set m for map m); d_values: int
	 * [npoly], or null for the values 0 .. npoly - 1; d_shifts: null, or double [nmaps][2], (dx, dy) of map m.  Map m is filled with
	 * `background`, then polygons 0 .. npoly - 1 are painted in that order with their values, later ones over earlier ones - bit for bit
	 * the reference's draw_polygon (geometry.cpp:81-152, DrawPolygon.h:180-398) on an int32 image, called once per polygon:
	 * vertices X = round(x + dx), Y = round(y + dy) in double (one addition, halves away from zero); 1 vertex: that pixel; 2 vertices:
	 * the reference's line (vertical, horizontal, x-major y = round(x * a + b), y-major x = round((y - b) / a), from the first point up
	 * to the second, which is drawn on its own); 3 or more: with B the vertices' bounding box [xmin, xmax + 1) x [ymin, ymax + 1), nothing
	 * when B misses the image, else every row Y0 of B clipped to the image: edge (i, j = i - 1) with Y_i != Y_j crosses where
	 * (Y_i < Y0 && Y_j >= Y0) || (Y_j < Y0 && Y_i >= Y0) - with <= for < on the clipped box's first row - at the node
	 * round(X_i + ((double)(Y0 - Y_i) / (Y_j - Y_i)) * (X_j - X_i)), every operation rounded on its own; the sorted nodes are filled in pairs
	 * (a, b): stop at the first a >= xmax, skip b < xmin, else max(a, xmin) .. min(b, xmax - 1).  On the first row equal neighbours are
	 * dropped first, in place in a buffer of npts + 1 zeros: the count is then at least 1 and an odd count pairs its last node with the
	 * entry after it (the sorted list's leftover, or 0) - so an apex draws its pixel, a polygon that is one horizontal run draws pixel
	 * (0, y) if it reaches column 0 and nothing otherwise, and identical vertices draw nothing.
	 * Deviation: the reference leaves huge and non-finite coordinates undefined; here a polygon draws nothing in a map where one of its
	 * shifted coordinates is not finite or exceeds 2^24 in magnitude.
	 * Every pixel of every map is written exactly once (no pre-fill needed), without atomics: bitwise reproducible.  npoly 0: background
	 * maps (d_xy, d_npts may be null).  nmaps 0: nothing is done.  Bounds: w, h >= 1, w * h <= 0x7FFF0000, 0 <= npoly <= 65536,
	 * 1 <= max_pts <= 1024.  d_work: device memory, 8-byte aligned, at least rir_polygon_map_workspace_bytes(...) (0: arguments refused).
	 * Asynchronous on `stream`; the maps and the workspace may not overlap an input or each other.  0 / -1 (invalid argument, null
	 * pointer, overlap, workspace too small, no device). */
	int rir_polygon_map_device(const double *d_xy, const int *d_npts, const int *d_values, int npoly, int max_pts, int nmaps, int sets_per_map,
							   const double *d_shifts, int w, int h, int background, int *d_dst, void *d_work, size_t work_bytes, void *stream);
	size_t rir_polygon_map_workspace_bytes(int w, int h, int nmaps, int npoly, int max_pts);

	/* connected components: reference signal_processing.h:90-92 / Filters.h:365-540 (labelImage, keepLargestArea) on images in device memory,
	 * [nframes][h][w], every image labelled on its own; five launches for the whole batch.  type: the reference's dtype character;
	 * background: HOST pointer to one cell of that type.  d_dst int32 [nframes][h][w].
	 * label: per image `table_entries` entries of d_xy (two doubles each: the first cell's x, twice - as upstream) and d_area, of which the
	 * first min(labels, table_entries) are written; d_count int[nframes] = labels = components + 1 (w*h + 1 entries are always enough);
	 * any memory the device can write.  d_work: device memory, 8-byte aligned, at least rir_label_workspace_bytes_batch(w, h, nframes)
	 * (0: geometry refused).  0 / -1.  The *_image_* forms are the batch of one with tables of w*h + 1 entries. */
	size_t rir_label_workspace_bytes(int w, int h);
	size_t rir_label_workspace_bytes_batch(int w, int h, int nframes);
	int rir_label_images_device(int type, const void *d_src, int *d_dst, int w, int h, int nframes, const void *background, double *d_xy, int *d_area,
								int table_entries, int *d_count, void *d_work, size_t work_bytes, void *stream);
	int rir_label_image_device(int type, const void *d_src, int *d_dst, int w, int h, const void *background, double *d_xy, int *d_area,
							   int *d_count, void *d_work, size_t work_bytes, void *stream);
	int rir_keep_largest_areas_device(int type, const void *d_src, int *d_dst, int w, int h, int nframes, const void *background, int foreground,
									  void *d_work, size_t work_bytes, void *stream);
	int rir_keep_largest_area_device(int type, const void *d_src, int *d_dst, int w, int h, const void *background, int foreground, void *d_work,
									 size_t work_bytes, void *stream);

	/* Hot spots labelled straight from the frames (extension): detection, filtering and numbering of the components of uint16 frames
	 * d_frames [nframes][h][w] above a threshold, without a mask in memory.  Pixel (y, x) of a frame is foreground when y < rows and its
	 * value v > low - d_low_map[y][x] when the map (int [h][w], shared by the frames) is given, else `low`; compared as int32, so a
	 * threshold < 0 takes every pixel and one >= 65535 none.  Components are the 4-connected sets of foreground pixels: what
	 * rir_label_images_device gives for the boolean mask.  A component is KEPT when all of these hold: use_high is 0, or it holds a pixel
	 * with v > high (d_high_map[y][x] when given, else `high`); min_area <= its pixel count <= max_area; clear_border is 0, or it has no
	 * pixel in row 0, row rows - 1, column 0 or column w - 1.  Kept components are numbered 1, 2, ... per frame in the raster order of
	 * their first pixel; pixels of dropped components and background pixels get 0 - d_dst int32 [nframes][h][w] is bit for bit the
	 * labelling of the mask of the kept components.  Per frame `table_entries` entries of d_area (pixel counts) and d_first (the raster
	 * index y * w + x of the component's first pixel), of which the first min(count, table_entries) are written, entry 0 being the
	 * background's (0, -1); d_count int[nframes] = kept components + 1.  Integer work, bitwise reproducible.  With no filter asked for
	 * (use_high 0, min_area 1, max_area >= w * h, clear_border 0) the launches are the five of rir_label_images_device; a filter adds
	 * one small pass over the roots - use_high and clear_border are gathered with the pixel counts, in no pass of their own.  Bounds: those of rir_label_images_device
	 * (w * h <= 0x7FFF0000, 1 <= nframes <= 65535), 1 <= rows <= h, 1 <= min_area <= max_area, table_entries >= 1.  d_work: device memory,
	 * 8-byte aligned, at least rir_label_hot_spots_workspace_bytes(w, h, nframes) (0: geometry refused).  Asynchronous on `stream`; no
	 * output or the workspace may overlap an input or another output.  0 / -1 (invalid argument, null pointer, overlap, workspace too
	 * small, no device). */
	size_t rir_label_hot_spots_workspace_bytes(int w, int h, int nframes);
	int rir_label_hot_spots_device(const unsigned short *d_frames, int w, int h, int nframes, int rows, int low, const int *d_low_map, int use_high,
								   int high, const int *d_high_map, int min_area, int max_area, int clear_border, int *d_dst, int *d_first, int *d_area,
								   int table_entries, int *d_count, void *d_work, size_t work_bytes, void *stream);

	/* ---- page-locked memory for the caller's images ------------------------------------------------------
	 * The reference's entry points take host pointers and hand the buffers back on return: every image crosses host memory
	 * once more than the link asks for (a copy into page-locked staging, a copy out of it).  A caller that keeps its images in memory
	 * from rir_host_alloc spares both: translate / gaussian_filter / bad_pixels_correct / rir_filter_chain / rir_gaussian_filter_u16 find such
	 * buffers (a registry of this library's blocks) and run their kernel on them in place.  The Python mirror returns its results in such
	 * memory, so the result of one call is the next call's input without a copy.  rir_host_alloc: NULL without a device or when the blocks
	 * handed out would exceed RIR_HOST_ALLOC_MAX_MB (256).  rir_host_free: only blocks of rir_host_alloc (anything else is left alone).
	 * rir_gaussian_filter_u16: gaussian_filter (reference signal_processing.cpp:79-148) of a uint16 image, bit-identical to converting it to
	 * float32 first as the reference's wrapper does (rir_signal_processing.py:85-113); radius <= 4, -1 otherwise. */
	void *rir_host_alloc(long long bytes);
	void rir_host_free(void *p);
	int rir_host_is_page_locked(const void *p, long long bytes);
	int rir_gaussian_filter_u16(unsigned short *src, float *dst, int w, int h, float sigma);

	/* ---- bounded-loss step on a device-resident stream -------------------------------------------------
	 * The loss injection of H264_Saver::addImageLossyNoCamera / addLoss (reference src/cpp/video_io/h264.cpp:2253-2607)
	 * as a stream operator: uint16 frames [n][h][w] in HBM in and out (distinct buffers), one state object per
	 * stream, frames taken in order.  rir_lossy_create returns a handle > 0 (0 on failure); low_errors /
	 * high_errors are HOST int[nframes] (the per-frame budgets, as h264_get_low/high_errors), may be NULL.
	 * Statistics, error budget and update all run on the device: the frames of a call are queued on `stream`
	 * back to back; with both arrays NULL the call returns without waiting, else it waits once, at the end. */
	int rir_lossy_create(int width, int height, int lossy_height, int low_value_error, int high_value_error, double std_factor,
						 int running_average, int subtract_min, int remove_bad_pixels);
	/* (the nframes input frames and the nframes output frames must not overlap: a run of frames reads input frames again - the frame
	 * that leaves the running average - after later outputs have been written; -1 otherwise) */
	int rir_lossy_step_device(int handle, const unsigned short *d_in, unsigned short *d_out, int nframes, int add_loss, int *low_errors,
							  int *high_errors, void *stream);
	/* The same step for nstreams INDEPENDENT streams (handles from rir_lossy_create with equal geometry, stepped the same number of
	 * frames so far, no bad-pixel repair) in shared launches: the state is sequential in time, so streams - not frames - are what
	 * runs side by side (SURVEY §8e "replicas").  d_in / d_out: HOST arrays of nstreams device pointers to uint16 [nframes][h][w];
	 * low_errors / high_errors: HOST int[nstreams][nframes] or NULL. */
	int rir_lossy_step_multi_device(const int *handles, int nstreams, const unsigned short *const *d_in, unsigned short *const *d_out, int nframes,
									int add_loss, int *low_errors, int *high_errors, void *stream);
	/* 0, or -1 when a run of frames this stream took part in gave up a wait between workgroups (a resident kernel that could not
	 * get all its workgroups on the chip).  Waits for `stream`.  The failure is STICKY: the stream's state has been advanced by
	 * invalid frames, so every later status and step of the stream - and of the streams that shared the failed call - returns -1
	 * until it is destroyed.  Calls that return budgets report this themselves; queue-only calls (no error arrays) leave it to
	 * this query. */
	int rir_lossy_status(int handle, void *stream);
	/* lowValueError / highValueError / stdFactor of a stream in use (H264_Saver::setParameter, h264.cpp:1709-1781): from the next frame on */
	int rir_lossy_set_errors(int handle, int low_value_error, int high_value_error, double std_factor);
	/* Which form stepped the last batch this stream led: out[0] = groups of frames offered to the constant-budget form (stdFactor == 0:
	 * the budget arithmetic of h264.cpp:2370-2376 multiplies the statistic by zero, so nothing a frame needs comes from another
	 * workgroup - an ordinary streaming launch instead of the resident one; 0 = the batch was not eligible), out[1] = of those, groups it
	 * took (it declines, on the device, when a frame's foreground or background may be empty or a NaN sits in the 40-frame window: then
	 * the general form steps the group, same results).  Waits for the stream. */
	int rir_lossy_path_stats(int handle, int *out2, void *stream);
	/* Streams whose budgets follow the statistics (stdFactor != 0 - the reference's default 5, h264.cpp:1662-1665, budget :2335-2385) go through
	 * the SPECULATIVE form: the budgets of a group are guessed (the configured errors: what a scene that does not move gets, the rounded correction
	 * being 0), the group is stepped by the streaming launch into shadow state, the frames' exact sums are taken from the frames and the reference's
	 * arithmetic is run for every frame; from the first frame whose budget is not the table's on, the table takes the computed budgets and the group
	 * is stepped again, up to RIR_LOSSY_SPEC_PASSES (3) times; a group that verifies is committed, any other is stepped by the general form - same
	 * results either way.
	 * out[0] = groups of the last batch this stream led that went through these launches (0: not eligible), out[1] = groups offered (no class that
	 * may be empty, no NaN in a window, the stream not backing off after failures), out[2] = groups committed, out[3] = passes over all groups.
	 * Waits for the stream. */
	int rir_lossy_spec_stats(int handle, int *out4, void *stream);
	void rir_lossy_destroy(int handle);

	/* ---- adaptive temporal downsampling (max-hold) on a device-resident stream -------------------------------
	 * VideoDownsampler (reference src/cpp/video_io/h264.cpp:117-451, h264.h:13-30), the event-driven recorder: out of a sequence about one
	 * image in `factor` is kept, more while the scene changes, and a kept image is the per-pixel maximum of everything since the last kept
	 * one, so a flash between two kept images is not lost.  uint16 frames [n][height][width] in HBM in, the kept images in HBM out.
	 * Parameters: 1 <= lossy_height <= height, S = width * lossy_height >= 2, factor >= 1, factor_std in [0, 1], method 1 (addImage) or
	 * 2 (addImage2); the history holds at most 96 statistics; part = (int)(factor_std * 96) clamped to 0..95.  Per image i, in order:
	 *   factor 1: the image is emitted as it is, nothing else is done.
	 *   statistic (i >= 1): over the first S pixels of images i and i - 1, d = |a - b|, x = sum d, q = sum d^2 as exact integers converted
	 *     to double once, stat = sqrt((q - (x * x) / S) / (S - 1)), every operation rounded on its own.
	 *   hold: max_im = max(max_im, image) over the first S pixels, rows from lossy_height on copied from the image.  An emission outputs
	 *     max_im for the current image (its time stamp and attributes go with it) and zeroes max_im: output k is the maximum over the
	 *     images after the previous kept one up to the keeping one, its rows below lossy_height are the keeping image's.  Image 0 is always
	 *     kept and emitted as itself.
	 *   method 1: while the history holds fewer than 96 entries, push stat (i > 0) and keep when i % factor == 0.  After that val = the
	 *     part-th smallest entry, (mean, std) = mean_std(history), nothing = stat < mean - 0.5 * std, false when i - last_added >= 2 * factor;
	 *     keep when (stat > val || i - last_added >= factor) && !nothing; then, when stat < mean + 10 * std, the oldest entry is dropped and
	 *     stat appended.
	 *   method 2: image 0 is kept.  While the history holds fewer than 10 entries, push stat and keep when i % factor == 0.  After that
	 *     nothing = (std / mean < 0.1) && stat < mean + 2 * std; keep when i % factor == 0 || (!nothing && stat > mean + 0.5 * std); the
	 *     history takes stat when (stat < mean + 5 * std && stat > mean - std) || i % factor == 0 - appended below 96 entries, else slid in.
	 *   mean_std: x += p, x2 += p * p in index order; x / n and sqrt((x2 - (x * x) / n) / (n - 1)).  A NaN result makes every comparison it
	 *     enters false, as in the reference.
	 * Deviations: (1) the sums are exact int64 - the reference accumulates in double, the same value while S * 65535^2 < 2^53, and squares
	 * in int, undefined for d > 46340; S > 2^31 - 1 is refused.  (2) A negative radicand of stat, which only the rounding of x * x can
	 * produce, gives 0 and not NaN (the reference would hand a NaN to std::nth_element): the history never holds a NaN.  (3) The reference
	 * refuses single images whose time stamp does not increase; here a push is refused as a whole, with nothing done, when its time stamps
	 * are not strictly increasing or do not exceed the last one pushed.  (4) Method 2 writes last_added and never reads it: not kept.
	 *
	 * rir_downsampler_create: a handle > 0 in the common handle namespace, 0 on failure (invalid argument, no device).
	 * rir_downsampler_push_device: the next nframes images of the stream; returns the number of images kept by this push (written to
	 * d_out[0 .. kept), capacity nframes images, which may not overlap d_frames), or -1 (invalid argument, time stamps, overlap, more than
	 * 4 194 240 images in one push with a factor above 1, no device: the state is untouched).  timestamps: HOST [nframes]; positions: HOST int[nframes], positions[k] = the index within this
	 * push of the image that triggered output k, whose time stamp and attributes go with it; stats: HOST double[nframes] or NULL,
	 * stats[i] = the statistic of image i, 0 for the very first image of the stream and for factor 1.  Two passes over the frames
	 * (pair sums, then the maxima of the kept images) with the recurrence on the host between them: the call waits ONCE for `stream`,
	 * after the first pass - which also serves the caller's queued work - and returns with the second pass queued.  Any split of a
	 * sequence into pushes gives the outputs, positions and statistics of one push of the whole; the state is the previous image and
	 * the running maximum (on the device), the history and the counters.  Integer work on the device, bitwise reproducible.  nframes 0: 0.
	 * rir_downsampler_count: images kept so far (what the reference's close() returns), -1 for an unknown handle. */
	int rir_downsampler_create(int width, int height, int lossy_height, int factor, double factor_std, int method);
	int rir_downsampler_push_device(int handle, const unsigned short *d_frames, int nframes, const long long *timestamps, unsigned short *d_out,
									int *positions, double *stats, void *stream);
	int rir_downsampler_count(int handle);
	void rir_downsampler_destroy(int handle);
	/* The recurrence alone, on the host, no device involved: sums[i] = {x, q} of image i (ignored for the first image of a stream),
	 * size = S; state: rir_downsample_state_bytes() bytes, 8-byte aligned, all zero for a stream that has seen nothing, carried from
	 * call to call; keep[i] = 1 where image i triggers an output; stats: [n] or NULL.  Returns the number kept, -1 on an invalid argument. */
	int rir_downsample_decide(int factor, double factor_std, int method, long long size, const long long *sums, int n, void *state, int *keep,
							  double *stats);
	size_t rir_downsample_state_bytes(void);

	/* ---- byte planes ------------------------------------------------------------------------------
	 * H264Capture::AddFrame (reference src/cpp/video_io/h264.cpp:1066-1082): U = v & 0xFF, V = v >> 8, Y = 0 or
	 * the 8-bit integration-time image, rows padded to `linesize`; VideoGrabber::toArray (:3016-3051) is the
	 * inverse.  Not on this build's own codec path (the block codec works on the 16-bit values); provided for
	 * callers that feed / read an external 8-bit plane codec.  Planes: [nframes][h][linesize]; d_it may be NULL. */
	int rir_split_planes_device(const unsigned short *d_img, const unsigned char *d_it, int w, int h, int nframes, int linesize,
								unsigned char *d_Y, unsigned char *d_U, unsigned char *d_V, void *stream);
	int rir_merge_planes_device(const unsigned char *d_Y, const unsigned char *d_U, const unsigned char *d_V, int linesize, int w, int h,
								int nframes, unsigned short *d_img, unsigned char *d_it, void *stream);

	/* ---- registration ---------------------------------------------------------------------------
	 * Translation-only ECC alignment, the arithmetic the reference obtains from OpenCV:
	 * cv2.findTransformECC(templ, image, warp, MOTION_TRANSLATION, (EPS|COUNT, max_iterations, eps), mask, 1)
	 * at src/python/librir/registration/masked_registration_ecc.py:166-168.  warp is a HOST float[2] = (tx, ty),
	 * start value in, result out: image(x + tx, y + ty) ~ templ(x, y).  *cc = correlation coefficient.
	 * Returns -1 where OpenCV raises (no overlap / no convergence). */
	int rir_ecc_translation_device(const float *d_templ, const float *d_image, const unsigned char *d_mask, int w, int h, float *warp,
								   int max_iterations, double eps, double *cc, int *iterations, void *stream);
	/* (im - min) / (max - min) in float32 on a w x h window of a device image with row stride src_stride (the
	 * normalisation of masked_registration_ecc.py:162-166, crop folded in); d_dst dense [h][w]. */
	int rir_minmax_normalize_device(const float *d_src, int w, int h, int src_stride, float *d_dst, void *stream);
	/* Pre-processing of `nframes` frames of a tracked sequence in shared launches, ahead of their (sequential) alignments: image
	 * by image the gaussian pre-filter, window crop, min-max normalisation (masked_registration_ecc.py:88-166) and the gradients
	 * the alignment samples.  d_imgs: uint16 ('H') or float32 ('f') [nframes][h][w]; d_norm, d_gx, d_gy: float
	 * [nframes][win_h][win_w] in device memory. */
	int rir_ecc_prepare_frames_device(const void *d_imgs, int dtype, int w, int h, int nframes, float sigma, int win_x, int win_y, int win_w, int win_h,
									  float *d_norm, float *d_gx, float *d_gy, void *stream);
	/* The alignment (cv2.findTransformECC, MOTION_TRANSLATION; masked_registration_ecc.py:166-168) of one prepared image against the
	 * reference window.  warp: HOST float[2] (tx, ty) in/out. */
	int rir_ecc_align_prepared_device(const float *d_ref_norm, const float *d_norm, const float *d_gx, const float *d_gy, int w, int h, float *warp,
									  int max_iterations, double eps, double *cc, int *iterations, void *stream);
	/* The alignments of `nframes` consecutive prepared images in one launch, image i starting from the result of image i - 1 (the
	 * loop of MaskedRegistratorECC.compute calls, masked_registration_ecc.py:102-123).  results: HOST [nframes][4] doubles = (tx, ty,
	 * correlation coefficient, iterations).  Returns how many images were aligned before the first failure (nframes: all), -1 on
	 * an invalid call.  warp: HOST float[2], start value in, last good result out. */
	int rir_ecc_align_prepared_frames_device(const float *d_ref_norm, const float *d_norm, const float *d_gx, const float *d_gy, int w, int h, int nframes,
											 float *warp, int max_iterations, double eps, double *results, void *stream);
	/* The alignments of nseq INDEPENDENT tracked sequences side by side in shared resident launches: for every sequence the
	 * operations of rir_ecc_align_prepared_frames_device in the same order (same bits), but S dependent chains at once instead of
	 * one - an alignment is a chain of iterations and cannot fill the chip on its own (masked_registration_ecc.py:105-191 is
	 * one such chain per camera).  All sequences share the window size w x h; d_ref_norm, d_norm, d_gx, d_gy: HOST arrays of nseq
	 * device pointers ([h][w] / [nframes[q]][h][w]); warps: HOST [nseq][2] in/out; results: HOST [nseq][results_stride][4]
	 * doubles (tx, ty, cc, iterations); good: HOST [nseq] = images of that sequence aligned before its first failure. */
	int rir_ecc_align_multi_device(const float *const *d_ref_norm, const float *const *d_norm, const float *const *d_gx, const float *const *d_gy, int w,
								   int h, int nseq, const int *nframes, float *warps, int max_iterations, double eps, double *results, int results_stride,
								   int *good, void *stream);
	/* The same with the pre-processing of what comes next UNDER the alignments: `next` = nnext jobs, each the arguments of one
	 * rir_ecc_prepare_frames_device call (normally the next chunk of every sequence).  The alignment launch needs the whole device to
	 * start, but once it is resident a fifth of every CU's places and most of the memory system are free: the library waits for the
	 * launch to report that and then runs the jobs on a stream of its own beside it; the caller's stream is ordered behind them when
	 * the call returns.  The jobs' outputs must not be buffers this call's alignments read. */
	typedef struct rir_ecc_prepare_job
	{
		const void *d_imgs;
		int dtype, w, h, nframes;
		float sigma;
		int win_x, win_y, win_w, win_h;
		float *d_norm, *d_gx, *d_gy;
	} rir_ecc_prepare_job;
	int rir_ecc_align_multi_overlapped_device(const float *const *d_ref_norm, const float *const *d_norm, const float *const *d_gx, const float *const *d_gy,
											  int w, int h, int nseq, const int *nframes, float *warps, int max_iterations, double eps, double *results,
											  int results_stride, int *good, const rir_ecc_prepare_job *next, int nnext, void *stream);
	/* One frame of a tracked sequence in one call - the steps of MaskedRegistratorECC.compute (masked_registration_ecc.py:88-168):
	 * gaussian pre-filter (sigma > 0), min-max normalisation of the registration window and the alignment against the
	 * already normalised reference window d_ref_norm [win_h][win_w], queued back to back with one read-back at the end.
	 * d_img: uint16 (dtype 'H') or float32 ('f') frame [h][w]. */
	int rir_ecc_register_frame_device(const void *d_img, int dtype, int w, int h, float sigma, int win_x, int win_y, int win_w, int win_h,
									  const float *d_ref_norm, float *warp, int max_iterations, double eps, double *cc, int *iterations,
									  void *stream);
	int find_transform_ecc_translation(const float *templ, const float *image, const unsigned char *mask, int w, int h, float *warp,
									   int max_iterations, double eps, double *cc);

	/* The host copy the per-frame entry points use between the caller's memory and page-locked staging (librir_amd/csrc/host_copy.cpp:
	 * a frame cut over a few helper threads; the reference's per-frame calls copy the caller's image the same way before they return,
	 * video_io.cpp:726-756 -> h264.cpp:1066-1082).  Plain host memory, no device involved: exported for tests and measurements.
	 * Returns the number of helper threads a copy may use (RIR_HOST_COPY_THREADS, default 3; 0 = memcpy on the calling thread), -1 on bad
	 * arguments. */
	int rir_host_copy(void *dst, const void *src, int64_t bytes);
	/* The same helpers move a chunk between page-locked memory and the container file (the saver's writer, the loader's read-ahead):
	 * write != 0 writes buf to [file_off, file_off + bytes) of the descriptor, else reads that range - all of it, or -1.  0 on success. */
	int rir_host_file_rw(int fd, void *buf, int64_t bytes, int64_t file_off, int write);
	/* first touch of [buf, buf + bytes) - fresh host memory that is being filled, e.g. the stack a slice of a movie is read into - one atomic
	 * compare-and-swap of a byte with itself per page on the calling thread (meant to run on a thread of its own, ahead of the reads); contents are left as they are. */
	int rir_host_touch(void *buf, int64_t bytes);

#ifdef __cplusplus
}
#endif
#endif /* RIR_AMD_DEVICE_H */
