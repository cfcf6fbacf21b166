"""Mirror of librir's ``signal_processing`` Python package (reference
src/python/librir/signal_processing/__init__.py) over the HIP shared object."""
from .BadPixels import BadPixels
from .rir_signal_processing import (bad_pixels_correct, bad_pixels_create, bad_pixels_destroy, distance_transform, extract_times, filter_chain,
                                    find_median_pixel, gaussian_filter, keep_largest_area, label_image, local_stats, local_threshold, morphology,
                                    pixel_quantiles, pixel_stats, polygon_map,
                                    percentile_rank, rank_filter, region_geometry, region_histogram, region_quantiles, region_stats,
                                    resample_time_serie, temporal_median, translate,
                                    fill_holes, h_dome, h_maxima, reconstruct)

__all__ = ["BadPixels", "translate", "gaussian_filter", "find_median_pixel", "bad_pixels_create", "bad_pixels_correct",
           "bad_pixels_destroy", "extract_times", "resample_time_serie", "label_image", "keep_largest_area", "filter_chain",
           "temporal_median", "region_stats", "pixel_stats", "polygon_map", "region_quantiles",
           "pixel_quantiles", "region_geometry", "morphology", "rank_filter", "percentile_rank", "region_histogram",
           "distance_transform", "local_stats", "local_threshold", "reconstruct", "h_maxima", "h_dome", "fill_holes"]
