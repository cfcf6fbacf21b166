"""CPU: what the Python forms of the frame filters - the temporal median, morphology, the rank filters, the local window statistics, the
distance transform, grey-level reconstruction and the regional extrema, in ``librir_amd.device`` over tensors and in
``librir_amd.signal_processing`` over arrays - answer to a bad call equals the record in tests/golden/frame_filter_messages.json, which was
made before the forms were given one stack intake, one test of ``out`` and one call tail.  The other tests ask only that a bad call is
refused; this one pins the exception type and the words and, with the calls that are wrong in two ways at once, the order in which the
conditions are tested: parameters, marker, ``out``, frames (``temporal_median``: the frames before ``out``).  CPU tensors serve: every
check in question comes before any device work.  The bad parameters of ``morphology`` and ``rank_filter`` themselves are in
window_filter_messages.json (test_window_filter_messages_cpu.py) and are not repeated here.

The "no_device" group - what a good host call answers where there is no device - is compared only on such a machine.

``PYTHONPATH=. python tests/test_frame_filter_messages_cpu.py`` writes the "cpu" group (and, without a device, "no_device") anew from the
library as it is and keeps the "gpu" group (test_gpu_frame_filter_forms.py)."""
import json
import os

import numpy as np

import test_distance_transform_cpu as DT
import test_local_stats_cpu as L
import test_morphology_cpu as M
import test_rank_filter_cpu as R
import test_reconstruct_cpu as RC

RECORD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "frame_filter_messages.json")

TEMPORAL_BAD = [dict(window=4), dict(window=65), dict(window=0), dict(threshold=-1), dict(threshold=65536), dict(rows=5), dict(rows=-1)]
TEMPORAL_BAD_DEVICE = [dict(first=7), dict(first=-1), dict(count=7), dict(count=-1), dict(step=0)]  # (the host form has no such parameters)
WINDOW_BAD = [c for c in M.BAD_PARAMETERS if "op" not in c]  # size and rows, as the aliases take them
RECONSTRUCT_BAD = [c for c in RC.BAD_PARAMETERS if "h" not in c]
SHIFT_BAD = [c for c in RC.BAD_PARAMETERS if "method" not in c]
BORDER_BAD = [c for c in RC.BAD_PARAMETERS if "method" not in c and "h" not in c]

# form -> (a good call's keywords, its bad parameters, the frames' dtype, the dtype of ``out`` - None: the form takes none)
DEVICE_FORMS = {
    "temporal_median": (dict(window=3, threshold=0, rows=None), TEMPORAL_BAD + TEMPORAL_BAD_DEVICE, "uint16", "uint16"),
    "morphology": (dict(op="open", size=3, rows=None), [], "uint16", "uint16"),
    "dilate": (dict(size=3, rows=None), WINDOW_BAD, "uint16", "uint16"),
    "rank_filter": (dict(rank=4, size=3, rows=None), [], "uint16", "uint16"),
    "window_median": (dict(size=3, rows=None), WINDOW_BAD, "uint16", "uint16"),
    "percentile_filter": (dict(percent=25, size=3, rows=None), WINDOW_BAD + [dict(percent=101), dict(percent=-101)], "uint16", "uint16"),
    "local_stats": (dict(size=3, rows=None), L.BAD_SHARED, "uint16", "int32"),
    "box_sum": (dict(size=3, rows=None), L.BAD_SHARED, "uint16", "int32"),
    "box_mean": (dict(size=3, rows=None), L.BAD_SHARED, "uint16", "uint16"),
    "local_threshold": (dict(size=3, k=3, delta=0, polarity="above", rows=None), L.BAD_SHARED + L.BAD_THRESHOLD, "uint16", "bool"),
    "distance_transform": (dict(background=0, border=False, rows=None), DT.BAD_PARAMETERS, "uint8", "int32"),
    "disc_erode": (dict(radius=2, border=False), [c for c in DT.BAD_PARAMETERS if "border" in c] + [dict(radius=-1), dict(radius=None)], "uint8", None),
    "reconstruct": (dict(method="dilation", connectivity=8, rows=None), RECONSTRUCT_BAD, "uint16", "uint16"),
    "h_maxima": (dict(h=3, connectivity=8, rows=None), SHIFT_BAD, "uint16", "uint16"),
    "h_dome": (dict(h=3, connectivity=8, rows=None), SHIFT_BAD, "uint16", "uint16"),
    "h_minima": (dict(h=3, connectivity=8, rows=None), SHIFT_BAD, "uint16", "uint16"),
    "h_basin": (dict(h=3, connectivity=8, rows=None), SHIFT_BAD, "uint16", "uint16"),
    "fill_holes": (dict(connectivity=4, rows=None), BORDER_BAD, "uint16", "uint16"),
    "clear_border": (dict(connectivity=8, rows=None), BORDER_BAD, "uint16", "uint16"),
    "regional_maxima": (dict(connectivity=8, rows=None), BORDER_BAD, "uint16", "bool"),
    "regional_minima": (dict(connectivity=8, rows=None), BORDER_BAD, "uint16", "bool"),
}
HOST_FORMS = ("temporal_median", "morphology", "rank_filter", "local_stats", "local_threshold", "reconstruct", "h_maxima", "h_dome", "fill_holes",
              "distance_transform")


def label(change):
    return ",".join("%s=%s" % kv for kv in change.items())


def raised(call):
    try:
        got = call()
    except Exception as e:  # noqa: BLE001  (the type is what is recorded)
        return [type(e).__name__, str(e)]
    return ["returned", described(got)]


def described(got):
    """dtype and shape of what a call returned (of every member of a tuple)"""
    if isinstance(got, tuple):
        return ", ".join(described(g) for g in got)
    return "%s %s" % (str(got.dtype).replace("torch.", ""), tuple(got.shape)) if hasattr(got, "dtype") else repr(got)


def call_form(module, name, data, kw, **more):
    """module.<name> over `data` with the keywords `kw`; a ``dtype`` among them is that of the data, not a parameter"""
    kw = dict({k: v for k, v in kw.items() if k != "dtype"}, **more)
    if name == "reconstruct":
        kw.setdefault("marker", data)
        return module.reconstruct(mask=data, **kw)
    return getattr(module, name)(data, **kw)


def python_answers():
    """{"<form> <what is wrong>": [exception type, message], or ["returned", dtypes and shapes]}"""
    import torch

    from librir_amd import device as D
    from librir_amd import signal_processing as S

    def tensor(shape, dtype):
        return torch.zeros(shape, dtype=getattr(torch, dtype))  # (a CPU tensor: the checks come before any device work)

    out = {}
    for name, (good, bad, dtype, out_dtype) in DEVICE_FORMS.items():
        # bad parameters: a stack, one image, the host form
        for change in bad:
            kw = dict(good, **change)
            dt = kw.get("dtype", dtype)
            out["device.%s %s" % (name, label(change))] = raised(lambda: call_form(D, name, tensor((6, 4, 5), dt), kw))
            out["device, one image.%s %s" % (name, label(change))] = raised(lambda: call_form(D, name, tensor((4, 5), dt), kw))
            if name in HOST_FORMS and change not in TEMPORAL_BAD_DEVICE:
                out["signal_processing.%s %s" % (name, label(change))] = raised(lambda: call_form(S, name, np.zeros((6, 4, 5), dt), kw))
        # an otherwise good call on CPU frames
        small = tensor((2, 4, 5), dtype)
        out["device.%s CPU frames" % name] = raised(lambda: call_form(D, name, small, good))
        out["device.%s CPU frames, one image" % name] = raised(lambda: call_form(D, name, small[0], good))
        if out_dtype is None:
            continue
        # a wrong 'out' (on CPU frames, which are looked at after it; by temporal_median before it)
        other = "int32" if out_dtype != "int32" else "uint16"
        wrong = {"of another dtype": tensor((2, 4, 5), other), "of another width": tensor((2, 4, 6), out_dtype), "of one image fewer": tensor((1, 4, 5), out_dtype),
                 "not contiguous": tensor((2, 4, 10), out_dtype)[:, :, ::2], "on the host": tensor((2, 4, 5), out_dtype), "the int 5": 5,
                 "a list": [1, 2]}
        if name == "local_stats":
            wrong = {what: (t, None, None) for what, t in wrong.items()}
            wrong.update({"no tuple: the int 5": 5, "no tuple: a tensor": tensor((2, 4, 5), "int32"), "a tuple of two": (tensor((2, 4, 5), "int32"),) * 2,
                          "a tuple of five": (None,) * 5})
            out["device.local_stats out with a wrong mean"] = raised(lambda: D.local_stats(small, 3, mean=True, out=(tensor((2, 4, 5), "int32"), None,
                                                                                                                    tensor((2, 4, 5), "uint8"))))
            out["device.local_stats out with no sum"] = raised(lambda: D.local_stats(small, 3, out=(None, None, None)))
        if name == "distance_transform":
            for what, t in list(wrong.items()):
                out["device.distance_transform, indices, out a pair, the first %s" % what] = raised(
                    lambda: D.distance_transform(small, return_indices=True, out=(t, tensor((2, 4, 5), "int32"))))
            wrong["a pair where one tensor is due"] = (tensor((2, 4, 5), "int32"),) * 2
            out["device.distance_transform, indices, out one tensor where a pair is due"] = raised(
                lambda: D.distance_transform(small, return_indices=True, out=tensor((2, 4, 5), "int32")))
            out["device.distance_transform, indices, out three tensors"] = raised(
                lambda: D.distance_transform(small, return_indices=True, out=(tensor((2, 4, 5), "int32"),) * 3))
        if name == "local_threshold":  # (both are taken: what is said next names the dtype that was picked)
            wrong.update({"uint8": tensor((2, 4, 5), "uint8"), "bool": tensor((2, 4, 5), "bool"), "uint8 of another width": tensor((2, 4, 6), "uint8")})
        for what, t in wrong.items():
            out["device.%s out %s" % (name, what)] = raised(lambda: call_form(D, name, small, good, out=t))
        out["device.%s out of another dtype, one image" % name] = raised(lambda: call_form(D, name, small[0], good, out=wrong["of another dtype"]))
        out["device.%s out of a stack for one image" % name] = raised(lambda: call_form(D, name, small[0], good, out=tensor((1, 4, 5), out_dtype)))
        # wrong in two ways at once: what is reported is what is tested first
        for change in bad[:1] + bad[-1:] if bad else [dict(rows=9)]:
            kw = dict(good, **change)
            dt = kw.get("dtype", dtype)
            out["device.%s %s, out of another dtype" % (name, label(change))] = raised(
                lambda: call_form(D, name, tensor((2, 4, 5), dt), kw, out=wrong["of another dtype"]))
            out["device.%s %s, out the int 5" % (name, label(change))] = raised(lambda: call_form(D, name, tensor((2, 4, 5), dt), kw, out=wrong["the int 5"]))
    # the marker of reconstruct, in both modules
    mask, images = tensor((2, 4, 5), "uint16"), np.zeros((2, 4, 5), np.uint16)
    for what, t, a in (("of another dtype", tensor((2, 4, 5), "uint8"), np.zeros((2, 4, 5), np.uint8)),
                       ("of another shape", tensor((2, 4, 6), "uint16"), np.zeros((2, 4, 6), np.uint16)),
                       ("one image for a stack", tensor((4, 5), "uint16"), np.zeros((4, 5), np.uint16)), ("the int 5", 5, 5), ("None", None, None)):
        out["device.reconstruct marker %s" % what] = raised(lambda: D.reconstruct(t, mask))
        out["device.reconstruct marker %s, out of another dtype" % what] = raised(lambda: D.reconstruct(t, mask, out=tensor((2, 4, 5), "int32")))
        out["device.reconstruct marker %s, connectivity=6" % what] = raised(lambda: D.reconstruct(t, mask, connectivity=6))
        out["signal_processing.reconstruct marker %s" % what] = raised(lambda: S.reconstruct(a, images))
        out["signal_processing.reconstruct marker %s, connectivity=6" % what] = raised(lambda: S.reconstruct(a, images, connectivity=6))
    out["device.reconstruct marker an array"] = raised(lambda: D.reconstruct(images, mask))
    # temporal_median: the one form that looks at the frames before 'out'
    out["device.temporal_median uint8 frames, out of another dtype"] = raised(
        lambda: D.temporal_median(tensor((2, 4, 5), "uint8"), 3, out=tensor((2, 4, 5), "int32")))
    out["device.temporal_median count=1, out of two images"] = raised(lambda: D.temporal_median(mask, 3, count=1, out=tensor((2, 4, 5), "uint16")))
    # what the host forms refuse as a stack, and what they return for an empty one
    for name in HOST_FORMS:
        good, _, dtype, _ = DEVICE_FORMS[name]
        for what, data in (("four dimensions", np.zeros((2, 2, 4, 5), dtype)), ("a row", np.zeros(5, dtype)), ("float64", np.zeros((2, 4, 5), np.float64)),
                           ("a list of lists", [[1, 2], [3, 4]]), ("None", None)):
            out["signal_processing.%s images: %s" % (name, what)] = raised(lambda: call_form(S, name, data, good))
        out["signal_processing.%s an empty stack" % name] = raised(lambda: call_form(S, name, np.zeros((0, 4, 5), dtype), good))
    out["signal_processing.local_stats an empty stack, every output"] = raised(
        lambda: S.local_stats(np.zeros((0, 4, 5), np.uint8), 3, sum=True, sumsq=True, mean=True))
    out["signal_processing.distance_transform an empty stack, indices"] = raised(
        lambda: S.distance_transform(np.zeros((0, 4, 5), np.uint8), return_indices=True))
    return out


def no_device_answers():
    """{"<form>": [exception type, message]} of an otherwise good host call, where there is no device"""
    from librir_amd import signal_processing as S

    return {"signal_processing.%s" % name: raised(lambda: call_form(S, name, np.zeros((2, 4, 5), DEVICE_FORMS[name][2]), DEVICE_FORMS[name][0]))
            for name in HOST_FORMS}


def compare(got, recorded):
    assert sorted(got) == sorted(recorded)
    different = {k: (v, recorded[k]) for k, v in got.items() if v != recorded[k]}
    assert not different, different


def write_group(group, answers):
    """the record with `group` replaced by `answers`"""
    record = {}
    if os.path.exists(RECORD):
        with open(RECORD) as f:
            record = json.load(f)
    record[group] = answers
    with open(RECORD, "w") as f:
        json.dump(record, f, indent=1, sort_keys=True)
        f.write("\n")


def test_refusals_are_worded_and_ordered_as_recorded(lib):
    with open(RECORD) as f:
        recorded = json.load(f)
    got = python_answers()
    compare(got, recorded["cpu"])
    returned = sorted(k for k, v in got.items() if v[0] == "returned")
    assert all("an empty stack" in k for k in returned) and len(returned) == len(HOST_FORMS) + 2, returned  # (nothing else gets through)


def test_host_forms_without_a_device_raise_as_recorded(lib):
    from librir_amd.device import device_available

    if device_available():
        import pytest

        pytest.skip("there is a device: the host forms answer")
    with open(RECORD) as f:
        recorded = json.load(f)["no_device"]
    got = no_device_answers()
    compare(got, recorded)
    for name in HOST_FORMS:
        assert got["signal_processing.%s" % name] == ["RuntimeError", "An error occured while calling '%s': librir_amd: no usable HIP device (this library "
                                                      "has no CPU fallback)" % name]


if __name__ == "__main__":
    from librir_amd.device import device_available

    write_group("cpu", python_answers())
    if not device_available():
        write_group("no_device", no_device_answers())
