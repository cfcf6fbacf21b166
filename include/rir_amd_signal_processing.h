/* librir_amd — the signal_processing C ABI of librir, served by HIP kernels on MI355X.
 *
 * Same symbol names, argument meaning and return codes as the reference header
 * src/cpp/signal_processing/signal_processing.h (cited per function), so that the library can be
 * loaded by librir's Python wrapper in place of libsignal_processing.so.
 * Host pointers in, host pointers out, synchronous.  No CPU fallback: every entry point that touches pixels runs on the device or
 * fails; extract_times / resample_time_serie / hash_bytes are host bookkeeping on timestamps and bytes and need none.
 */
#ifndef RIR_AMD_SIGNAL_PROCESSING_H
#define RIR_AMD_SIGNAL_PROCESSING_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C"
{
#endif

	/* reference signal_processing.h:29 — 0 on success, -1 on unknown dtype char / strategy.
	 * strategy: NULL, "", "noborder", "background", "wrap", "nearest".  dst is in/out. */
	int translate(int type, void *src, void *dst, int w, int h, float dx, float dy, void *background, const char *strategy);

	/* reference signal_processing.h:33 */
	int gaussian_filter(float *src, float *dst, int w, int h, float sigma);

	/* reference signal_processing.h:39,44 (the C++ default argument percent = 0.5 is explicit here) */
	int find_median_pixel(unsigned short *pixels, int size, float percent);
	int find_median_pixel_mask(unsigned short *pixels, unsigned char *mask, int size, float percent);

	/* reference signal_processing.h:80,84,88 — create returns the handle (>0) or 0 on error */
	int bad_pixels_create(unsigned short *first_image, int width, int height);
	int bad_pixels_correct(int handle, unsigned short *in, unsigned short *out);
	void bad_pixels_destroy(int handle);

	/* reference signal_processing.h:94 */
	size_t hash_bytes(void *ptr, size_t len);

	/* reference signal_processing.h:55 / signal_processing.cpp:158-181 — one time axis out of several (s: 0 union, 1 intersection).
	 * time_vector: the vectors one after the other, vector_sizes[vector_count] their lengths.  0; -2 with the needed size in
	 * *output_size when the output is too small; -1 on input the reference does not return from (csrc/time_series.cpp). */
	int extract_times(double *time_vector, int vector_count, int *vector_sizes, int s, double *output, int *output_size);
	/* reference signal_processing.h:71 / signal_processing.cpp:183-195 — (sample_x, sample_y) read at `times` (s: 2 pad with padds
	 * outside the samples, 4 interpolate).  0; -1 when the output is too small (needed size in *output_size). */
	int resample_time_serie(double *sample_x, double *sample_y, int size, double *times, int times_size, int s, double padds, double *output,
							int *output_size);
	/* reference signal_processing.h:90 / signal_processing.cpp:224-266 — connected components of `src` (cells != *background; joined
	 * vertically whatever their values, horizontally when equal), numbered from 1 in raster order of their first pixel into dst.
	 * Returns the number of table entries (components + 1; entry 0 is the background's) written to out_xy (x of the first pixel, twice -
	 * as upstream) and out_area, -1 on an unknown type. */
	int label_image(int type, void *src, int *dst, int w, int h, void *background, double *out_xy, int *out_area);
	/* reference signal_processing.h:92 / signal_processing.cpp:276-318 — dst = foreground on the largest component, (int)*background
	 * elsewhere (all zero without a component).  0, -1 on an unknown type. */
	int keep_largest_area(int type, void *src, int *dst, int w, int h, void *background, int foreground);

	/* ---- extension (prefix rir_) ----
	 * bad_pixels_correct -> gaussian_filter(sigma) -> translate(dx, dy, strategy) -> uint16 on one host image in ONE call: what a caller of the
	 * three entry points above does in three (BASELINE configs[2]), without the two float images in between.  bad_pixels_handle 0: no
	 * repair; strategy "nearest" or "background" (background: one uint16).  The three calls' result within one level, or exactly with
	 * rir_set_gaussian_reference_order(1) (rir_amd_device.h).  0 / -1. */
	int rir_filter_chain(int bad_pixels_handle, unsigned short *in, unsigned short *out, int w, int h, float sigma, float dx, float dy,
						 void *background, const char *strategy);
	/* Temporal median of a host stack src[nframes][h][w] into dst (same shape): rir_temporal_median_device over the whole stack (first 0,
	 * step 1), synchronous.  Large stacks go through the device in slabs with window / 2 frames of halo.  0 / -1. */
	int rir_temporal_median(const unsigned short *src, unsigned short *dst, int w, int h, int nframes, int window, int threshold, int rows);
	/* Flat morphology of a host stack src[nframes][h][w] into dst (same type and shape): rir_morphology_device (rir_amd_device.h) over the
	 * stack, synchronous.  type 'H' uint16, 'B' uint8, '?' bool; op 0 erode (min over the size_y x size_x window clipped to the image),
	 * 1 dilate (max), 2 open (dilate of erode), 3 close (erode of dilate), 4 tophat (src - open), 5 blackhat (close - src), 6 gradient
	 * (dilate - erode); sizes odd, 1..15; the image is the first `rows` (0..h) rows, the others are copied.  Large stacks go through the
	 * device in slabs of at most 64 MiB (frames are independent).  dst == src is allowed, any other overlap is not.  nframes 0: 0.
	 * -1 with the reason logged on a bad argument (before the device is looked for) and without a device ("no usable HIP device", dst
	 * untouched: there is no CPU fallback). */
	int rir_morphology(int type, const void *src, void *dst, int w, int h, int nframes, int op, int size_x, int size_y, int rows);
	/* Spatial rank filter of a host stack src[nframes][h][w] into dst (same type and shape): rir_rank_filter_device (rir_amd_device.h) over
	 * the stack, synchronous.  type 'H' uint16, 'B' uint8, '?' bool; sizes odd, 1..15; 0 <= rank < size_x * size_y.  With the image the
	 * first `rows` (0..h) rows (the others are copied), dst[n][y][x] = the element of 0-based rank `rank` among the size_y * size_x values
	 * src[n][clamp(y + dy, 0, rows - 1)][clamp(x + dx, 0, w - 1)], |dy| <= size_y / 2, |dx| <= size_x / 2: a full window with coordinates
	 * replicated at the border, scipy.ndimage.rank_filter(..., size=(size_y, size_x), mode="nearest") per frame.  Large stacks go through
	 * the device in slabs of at most 64 MiB (frames are independent).  dst == src is allowed, any other overlap is not.  nframes 0: 0.
	 * -1 with the reason logged on a bad argument (before the device is looked for) and without a device ("no usable HIP device", dst
	 * untouched: there is no CPU fallback). */
	int rir_rank_filter(int type, const void *src, void *dst, int w, int h, int nframes, int rank, int size_x, int size_y, int rows);
	/* Local window statistics of a host stack src[nframes][h][w]: rir_local_stats_device (rir_amd_device.h, where the outputs are defined)
	 * over the stack, synchronous.  sum (int32), sumsq (int64) and mean (the type of src) have the shape of src; each may be null, at least
	 * one must not be, and none may overlap src or another.  Large stacks go through the device in slabs of at most 64 MiB of the widest
	 * array (frames are independent).  nframes 0: 0.  -1 with the reason logged on a bad argument (before the device is looked for) and
	 * without a device ("no usable HIP device", the outputs untouched: there is no CPU fallback). */
	int rir_local_stats(int type, const void *src, int w, int h, int nframes, int size_x, int size_y, int rows, int *sum, long long *sumsq, void *mean);
	/* The z-score mask of a host stack src[nframes][h][w] into mask[nframes][h][w] (one byte 0 / 1 a pixel): rir_local_threshold_device
	 * (rir_amd_device.h, where the rule is defined) over the stack, synchronous, in slabs as rir_local_stats.  mask may not overlap src.
	 * 0 / -1 as rir_local_stats. */
	int rir_local_threshold(int type, const void *src, unsigned char *mask, int w, int h, int nframes, int size_x, int size_y, int rows, int k_num,
							int k_den, int delta, int polarity);
	/* Exact Euclidean distance transform of a host stack src[nframes][h][w]: rir_distance_transform_device (rir_amd_device.h, where the rule
	 * is defined) over the stack, synchronous.  type '?' bool, 'B' uint8, 'H' uint16, 'i' int32; a cell equal to `background` is
	 * background; dist2[nframes][h][w] (int32) is the squared distance to the nearest background pixel among the first `rows` (0..h) rows
	 * of the frame - with border 1 also to the outside of the image -, RIR_DIST2_NONE where there is none; index (int32, may be NULL) the
	 * lowest flat index y * w + x of such a pixel, -1 where there is none or the outside is strictly nearer.  1 <= w, h <= 16384.  Large
	 * stacks go through the device in slabs sized by a frame's input, outputs and workspace, 64 MiB each at most (frames are independent).
	 * No output may overlap the input or the other output.  nframes 0: 0.  -1 with the reason logged on a bad argument (before the device
	 * is looked for) and without a device ("no usable HIP device", outputs untouched: there is no CPU fallback). */
	int rir_distance_transform(int type, const void *src, int w, int h, int nframes, int background, int border, int rows, int *dist2, int *index);
	/* Grey-level morphological reconstruction of host stacks: rir_reconstruct_device (rir_amd_device.h, where the rule is defined) over
	 * mask[nframes][h][w] and, in marker mode 0, marker[nframes][h][w], synchronous.  type 'H' uint16, 'B' uint8, '?' bool; method 0
	 * dilation, 1 erosion; connectivity 4 or 8; marker_mode 0 explicit (marker must be NULL otherwise), 1 the mask shifted by param
	 * (0..the type's maximum, saturating), 2 the mask on the border of the image; output 0 the reconstruction R, 1 its difference to the
	 * mask; the image is the first `rows` (0..h) rows, the others are a copy of the mask.  *rounds (may be NULL): the largest number of
	 * rounds a slab took.  Large stacks go through the device in slabs of at most 64 MiB (frames are independent).  dst may overlap
	 * neither input; marker == mask is allowed.  nframes 0: 0.  -1 with the reason logged on a bad argument (before the device is looked
	 * for) and without a device ("no usable HIP device", dst untouched: there is no CPU fallback). */
	int rir_reconstruct(int type, const void *mask, const void *marker, void *dst, int w, int h, int nframes, int method, int connectivity,
						int marker_mode, int param, int output, int rows, int *rounds);
	/* Per-region statistics of a host stack frames[nframes][h][w] with host label maps: rir_region_stats_device (rir_amd_device.h),
	 * synchronous, host outputs [nframes][nregions].  The frames go through the device in slabs of at most 64 MiB; a shared map goes up
	 * once.  0 / -1. */
	int rir_region_stats(const unsigned short *frames, const int *labels, int w, int h, int nframes, int labels_per_frame, int nregions,
						 int *count, long long *sum, long long *sumsq, int *min, int *max, int *argmin, int *argmax);
	/* Per-region geometry of host label maps, weighted by a host stack frames[nframes][h][w] when `frames` is not null:
	 * rir_region_geometry_device (rir_amd_device.h, where the outputs are defined), synchronous, host outputs count[nframes][nregions],
	 * bbox[..][4], moments[..][5] and, with frames, weighted[..][3] (null exactly when frames is).  The frames and per-frame maps go
	 * through the device in slabs of at most 64 MiB; a shared map goes up once.  0 / -1. */
	int rir_region_geometry(const int *labels, const unsigned short *frames /* or null */, int w, int h, int nframes, int labels_per_frame,
							int nregions, int *count, int *bbox, long long *moments, long long *weighted /* null iff frames is null */);
	/* Per-region quantiles of a host stack frames[nframes][h][w] with host label maps: rir_region_quantiles_device (rir_amd_device.h, where
	 * the rule is defined), synchronous, host outputs count[nframes][nregions] and values[nframes][nregions][npercents].  The frames go
	 * through the device in slabs of at most 64 MiB; a shared map goes up once.  0 / -1. */
	int rir_region_quantiles(const unsigned short *frames, const int *labels, int w, int h, int nframes, int labels_per_frame, int nregions,
							 const float *percents, int npercents, int *count, int *values);
	/* Per-region histograms of a host stack frames[nframes][h][w] with host label maps, or none (labels null: the whole image is region 0,
	 * nregions 1): rir_region_histogram_device (rir_amd_device.h, where the bins are defined), synchronous, host outputs
	 * count[nframes][nregions], hist[nframes][nregions][nbins] and outside[nframes][nregions][2]; count and outside may be null.  The
	 * frames go through the device in slabs of at most 64 MiB; a shared map goes up once.  nframes 0: 0.  -1 with the reason logged on a
	 * bad argument (before the device is looked for) and without a device (the outputs untouched: there is no CPU fallback). */
	int rir_region_histogram(const unsigned short *frames, const int *labels /* or null */, int w, int h, int rows, int nframes,
							 int labels_per_frame, int nregions, int lo, int width, int nbins, int *count /* or null */, int *hist,
							 int *outside /* or null */);
	/* Per-pixel statistics over time of a host stack frames[nframes][h][w]: rir_pixel_stats_device (rir_amd_device.h) with t0 = 0,
	 * synchronous, host outputs [h][w]; a group (sum, sumsq / min, max, argmin, argmax) may be null, not both.  The frames go through the
	 * device in slabs of at most 64 MiB that accumulate there; the outputs come back once.  nframes 0: nothing is done.  0 / -1. */
	int rir_pixel_stats(const unsigned short *frames, int w, int h, int nframes, long long *sum, long long *sumsq, int *min, int *max,
						int *argmin, int *argmax);
	/* Per-pixel quantiles over time of a host stack frames[nframes][h][w]: rir_pixel_quantiles_device (rir_amd_device.h, where the rule is
	 * defined), synchronous, host output values[npercents][h][w].  A stack of at most 256 MiB goes up once; a larger one goes through the
	 * device in slabs of at most 64 MiB, once per pass, through the streaming form: the same bits.  nframes 0: -1 everywhere.  0 / -1. */
	int rir_pixel_quantiles(const unsigned short *frames, int w, int h, int nframes,
							const float *percents, int npercents, int *values);
	/* Polygon label maps into host memory dst[nmaps][h][w] from host polygons: rir_polygon_map_device (rir_amd_device.h, where the fill is
	 * defined), synchronous.  The polygons, values and shifts go up once; the maps come back in slabs of at most 64 MiB.  values and shifts
	 * may be null.  nmaps 0: nothing is done.  0 / -1. */
	int rir_polygon_map(const double *xy, const int *npts, const int *values, int npoly, int max_pts, int nmaps, int sets_per_map,
						const double *shifts, int w, int h, int background, int *dst);

#ifdef __cplusplus
}
#endif
#endif /* RIR_AMD_SIGNAL_PROCESSING_H */
