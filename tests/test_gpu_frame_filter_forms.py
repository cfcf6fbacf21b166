"""GPU: the Python forms of the frame filters in ``librir_amd.device`` as wrappers, at the smallest shapes at which a wrapper can go wrong - a
stack (2, 3, 5) and one image (3, 5): every form equals the host form of the same name bit for bit (where there is none, the composition its
docstring states), returns ``out`` itself when given one, takes a non-contiguous stack as its contiguous copy, gives an image for an image and
an empty tensor of the documented dtype for no frames, and passes on what the C entry says to an ``out`` that overlaps the input - the "gpu"
group of tests/golden/frame_filter_messages.json (see test_frame_filter_messages_cpu.py for what needs no device).  What the kernels compute
is the matter of test_gpu_morphology.py, test_gpu_rank_filter.py, test_gpu_local_stats.py, test_gpu_distance_transform.py,
test_gpu_reconstruct.py and test_gpu_temporal_median.py.

``PYTHONPATH=. python tests/test_gpu_frame_filter_forms.py`` on a machine with a device writes the "gpu" group anew and keeps the others."""
import json

import numpy as np
import pytest

import test_frame_filter_messages_cpu as C

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

TOP = {"uint16": 65535, "uint8": 255, "bool": 1, "int32": (1 << 31) - 1}
WINDOWED = ("uint16", "uint8", "bool")

# ``out is the returned object, with the same bits`` is asserted for these forms, at larger shapes, by test_gpu_morphology.py
# (test_every_op..., the aliases), test_gpu_rank_filter.py (rank_filter, window_median, percentile_filter), test_gpu_local_stats.py (local_stats,
# box_sum, box_mean), test_gpu_reconstruct.py::test_named_forms_equal_the_generic_one (the h_ forms, fill_holes, clear_border, the regional
# extrema; also an image for an image) and test_gpu_temporal_median.py::test_overlap_is_refused: not again here.
OUT_ASSERTED_ELSEWHERE = {"morphology", "dilate", "rank_filter", "window_median", "percentile_filter", "local_stats", "box_sum", "box_mean", "h_maxima",
                          "h_dome", "h_minima", "h_basin", "fill_holes", "clear_border", "regional_maxima", "regional_minima", "temporal_median"}


def dev(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:
        return torch.from_numpy(a.view(np.int16)).cuda().view(torch.uint16)
    return torch.from_numpy(a).cuda()


def host(t):
    if isinstance(t, tuple):
        return tuple(None if m is None or isinstance(m, int) else host(m) for m in t)
    if t.dtype == torch.uint16:
        return t.cpu().view(torch.int16).numpy().view(np.uint16)
    return t.cpu().numpy()


def same(got, want):
    if isinstance(want, tuple):
        return len(got) == len(want) and all((g is None and w is None) or (g is not None and w is not None and same(g, w)) for g, w in zip(got, want))
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want)


def pattern(shape, dtype):
    """a few levels with plateaus, extrema inside and on the border, the same for every call"""
    v = (np.arange(int(np.prod(shape)), dtype=np.int64) * 7919 + 3) % 11
    v = v.reshape(shape)
    return (v > 4) if dtype == "bool" else (v * (TOP[dtype] // 13)).astype(dtype)


def saturated(a, shift):
    return np.clip(a.astype(np.int64) + shift, 0, TOP[a.dtype.name]).astype(a.dtype)


def border_marker(a, inside):
    m = np.full_like(a, inside)
    for edge in (np.s_[..., 0, :], np.s_[..., -1, :], np.s_[..., :, 0], np.s_[..., :, -1]):
        m[edge] = a[edge]
    return m


def h_of(a):
    return 1 if a.dtype == np.bool_ else TOP[a.dtype.name] // 13 * 2


def difference(a, b):
    return (a ^ b) if a.dtype == np.bool_ else (a - b)


def h_minima(S, a, h):
    return S.reconstruct(saturated(a, h), a, "erosion")


def stats3(s):
    return (s.sum, s.sumsq, s.mean)


# form -> (the dtypes it is run on, call(D, frames, out) on the device, the same on the host from the module S and the array a)
FORMS = {
    "temporal_median": (("uint16",), lambda D, f, out: D.temporal_median(f, 3, 2, out=out), lambda S, a: S.temporal_median(a.reshape((-1,) + a.shape[-2:]), 3, 2)),
    "morphology": (WINDOWED, lambda D, f, out: D.morphology(f, "gradient", (3, 1), out=out), lambda S, a: S.morphology(a, "gradient", (3, 1))),
    "dilate": (WINDOWED, lambda D, f, out: D.dilate(f, 3, 2, out=out), lambda S, a: S.morphology(a, "dilate", 3, 2)),
    "rank_filter": (WINDOWED, lambda D, f, out: D.rank_filter(f, -2, (1, 3), out=out), lambda S, a: S.rank_filter(a, -2, (1, 3))),
    "window_median": (WINDOWED, lambda D, f, out: D.window_median(f, 3, out=out), lambda S, a: S.rank_filter(a, 4, 3)),
    "percentile_filter": (WINDOWED, lambda D, f, out: D.percentile_filter(f, 25, (3, 5), out=out),
                          lambda S, a: S.rank_filter(a, S.percentile_rank(25, 3, 5), (3, 5))),
    "local_stats": (WINDOWED, lambda D, f, out: stats3(D.local_stats(f, 3, sumsq=True, mean=True, out=out)),
                    lambda S, a: stats3(S.local_stats(a, 3, sumsq=True, mean=True))),
    "box_sum": (WINDOWED, lambda D, f, out: D.box_sum(f, (3, 1), out=out), lambda S, a: S.local_stats(a, (3, 1)).sum),
    "box_mean": (WINDOWED, lambda D, f, out: D.box_mean(f, 3, 2, out=out), lambda S, a: S.local_stats(a, 3, 2, sum=False, mean=True).mean),
    "local_threshold": (WINDOWED, lambda D, f, out: D.local_threshold(f, 3, (1, 2), polarity="both", out=out),
                        lambda S, a: S.local_threshold(a, 3, (1, 2), polarity="both")),
    "distance_transform": (("bool", "uint8", "uint16", "int32"), lambda D, f, out: D.distance_transform(f, border=True, out=out),
                           lambda S, a: S.distance_transform(a, border=True)),
    "distance_transform, indices": (("uint8",), lambda D, f, out: D.distance_transform(f, return_indices=True, out=out),
                                    lambda S, a: S.distance_transform(a, return_indices=True)),
    "disc_erode": (("bool", "uint8"), lambda D, f, out: D.disc_erode(f, 1),
                   lambda S, a: ((a != 0) & (S.distance_transform(a) > 1)).astype(a.dtype)),
    "reconstruct": (WINDOWED, lambda D, f, out: D.reconstruct(dev(saturated(host(f), -h_of(host(f)))), f, connectivity=4, out=out),
                    lambda S, a: S.reconstruct(saturated(a, -h_of(a)), a, connectivity=4)),
    "h_maxima": (WINDOWED, lambda D, f, out: D.h_maxima(f, h_of(host(f)), out=out), lambda S, a: S.h_maxima(a, h_of(a))),
    "h_dome": (WINDOWED, lambda D, f, out: D.h_dome(f, h_of(host(f)), 4, out=out), lambda S, a: S.h_dome(a, h_of(a), 4)),
    "h_minima": (WINDOWED, lambda D, f, out: D.h_minima(f, h_of(host(f)), out=out), lambda S, a: h_minima(S, a, h_of(a))),
    "h_basin": (WINDOWED, lambda D, f, out: D.h_basin(f, h_of(host(f)), out=out), lambda S, a: difference(h_minima(S, a, h_of(a)), a)),
    "fill_holes": (WINDOWED, lambda D, f, out: D.fill_holes(f, out=out), lambda S, a: S.fill_holes(a)),
    "clear_border": (WINDOWED, lambda D, f, out: D.clear_border(f, out=out), lambda S, a: difference(a, S.reconstruct(border_marker(a, 0), a))),
    "regional_maxima": (WINDOWED, lambda D, f, out: D.regional_maxima(f, out=out), lambda S, a: S.h_dome(a, 1) != 0),
    "regional_minima": (WINDOWED, lambda D, f, out: D.regional_minima(f, out=out), lambda S, a: difference(h_minima(S, a, 1), a) != 0),
}
NO_OUT = ("disc_erode",)


def like(got):
    """new tensors of the dtypes and shapes of a result (None where it has none)"""
    if isinstance(got, tuple):
        return tuple(None if t is None else torch.empty_like(t) for t in got)
    return torch.empty_like(got)


@pytest.mark.parametrize("name", sorted(FORMS))
def test_form_equals_its_host_twin_on_stacks_views_images_and_no_frames(name):
    from librir_amd import device as D
    from librir_amd.signal_processing import rir_signal_processing as S

    dtypes, form, twin = FORMS[name]
    for dtype in dtypes:
        a = pattern((2, 3, 5), dtype)
        want = twin(S, a)
        got = form(D, dev(a), None)
        assert same(host(got), want), dtype
        if name not in NO_OUT and name not in OUT_ASSERTED_ELSEWHERE:
            out = like(got)
            back = form(D, dev(a), out)
            assert (all(b is o for b, o in zip(back, out)) if isinstance(out, tuple) else back is out) and same(host(back), want), dtype
        wide = dev(np.repeat(a, 2, axis=2))[:, :, ::2]
        assert not wide.is_contiguous() and same(host(form(D, wide, None)), want), dtype
        image = form(D, dev(a[0]), None)
        one = twin(S, a[0]) if name != "temporal_median" else twin(S, a[:1])  # (temporal_median documents [count][h][w]: one image is a stack of one)
        assert same(host(image), one), dtype
        empty = form(D, dev(a[:0]), None)
        for e, g in zip(empty, got) if isinstance(got, tuple) else ((empty, got),):
            assert e.is_cuda and e.dtype == g.dtype and tuple(e.shape) == (0, 3, 5), (dtype, e.shape)


def overlapping(*dtypes):
    """a stack (2, 3, 5) of each dtype, all starting at the same address"""
    raw = torch.zeros(2 * 3 * 5, dtype=torch.int64, device="cuda").view(torch.uint8)
    return tuple(raw[:30 * torch.empty((), dtype=dt).element_size()].view(dt).view(2, 3, 5) for dt in dtypes)


def gpu_answers():
    """{"device.<form> out overlaps the input": [exception type, message]}: the C entry's words, through ``_check``"""
    from librir_amd import device as D

    u16, u8, i32 = torch.uint16, torch.uint8, torch.int32
    got = {}
    for name, (good, _, dtype, out_dtype) in C.DEVICE_FORMS.items():
        if out_dtype is None or name.startswith("regional_"):  # (the regional extrema hand their 'out' to torch.ne, not to the C entry)
            continue
        f, out = overlapping(getattr(torch, dtype), getattr(torch, out_dtype))
        out = (out, None, None) if name == "local_stats" else out
        got["device.%s out overlaps the input" % name] = C.raised(lambda: C.call_form(D, name, f, good, out=out))
    f, out = overlapping(u16, u16)
    got["device.reconstruct out overlaps the marker"] = C.raised(lambda: D.reconstruct(f, torch.zeros_like(f), out=out))
    f, out = overlapping(u16, u8)
    got["device.local_threshold uint8 out overlaps the input"] = C.raised(lambda: D.local_threshold(f, 3, 1, out=out))
    f, out = overlapping(u8, i32)
    got["device.distance_transform index overlaps the input"] = C.raised(lambda: D.distance_transform(f, return_indices=True, out=(torch.empty_like(out), out)))
    got["device.distance_transform index overlaps dist2"] = C.raised(lambda: D.distance_transform(torch.zeros_like(f), return_indices=True, out=(out, out)))
    f, total, mean = overlapping(u16, i32, u16)
    got["device.local_stats out.mean overlaps the input"] = C.raised(lambda: D.local_stats(f, 3, mean=True, out=(torch.empty_like(total), None, mean)))
    return got


def test_an_out_that_overlaps_the_input_is_refused_in_the_words_of_the_c_entry():
    with open(C.RECORD) as f:
        recorded = json.load(f)["gpu"]
    got = gpu_answers()
    C.compare(got, recorded)
    assert all(v[0] == "RuntimeError" and "_device failed: " in v[1] for v in got.values()), got


def test_what_the_cpu_record_cannot_reach_about_out():
    from librir_amd import device as D

    frames = dev(pattern((2, 3, 5), "uint16"))
    # temporal_median looks at the frames first: its 'out' is reached on the device only
    for wrong in (5, [1, 2], torch.empty((2, 3, 5), dtype=torch.uint16), torch.empty((2, 3, 5), dtype=torch.int32, device="cuda"),
                  torch.empty((2, 3, 10), dtype=torch.uint16, device="cuda")[:, :, ::2]):
        with pytest.raises(RuntimeError, match=r"^temporal_median: out must be a contiguous uint16 CUDA tensor of shape \(2, 3, 5\)$"):
            D.temporal_median(frames, 3, out=wrong)
    # the other forms refuse an 'out' that is right but for its strides; the regional extrema take it
    strided = torch.empty((2, 3, 10), dtype=torch.uint16, device="cuda")[:, :, ::2]
    with pytest.raises(RuntimeError, match="^morphology: out must be a contiguous"):
        D.morphology(frames, "open", 3, out=strided)
    with pytest.raises(RuntimeError, match="^h_dome: out must be a contiguous"):
        D.h_dome(frames, 3, out=strided)
    with pytest.raises(RuntimeError, match="^distance_transform: out must be a contiguous"):
        D.distance_transform(frames, out=torch.empty((2, 3, 10), dtype=torch.int32, device="cuda")[:, :, ::2])
    found = torch.zeros((2, 3, 10), dtype=torch.bool, device="cuda")[:, :, ::2]
    assert D.regional_maxima(frames, out=found) is found and torch.equal(found, D.regional_maxima(frames)) and found.any()
    # local_threshold writes 0 / 1 into a uint8 'out' as it does into a bool one
    mask = D.local_threshold(frames, 3, 0)
    bytes_out = torch.full((2, 3, 5), 7, dtype=torch.uint8, device="cuda")
    assert D.local_threshold(frames, 3, 0, out=bytes_out) is bytes_out and torch.equal(bytes_out, mask.view(torch.uint8)) and mask.any()


if __name__ == "__main__":
    C.write_group("gpu", gpu_answers())
