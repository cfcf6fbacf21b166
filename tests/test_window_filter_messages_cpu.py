"""CPU: what morphology and the rank filters answer to a bad call - the return value and the full error text of both C entries of each
filter, the exception type and message of the Python forms - equals the record in tests/golden/window_filter_messages.json, which was made
before the two families' argument checks were merged.  The other tests ask only that a bad call is refused; this one pins the words and, with
the calls that are wrong in two ways at once, the order in which the conditions are tested.  Needs no device: every check comes before it.

``PYTHONPATH=. python tests/test_window_filter_messages_cpu.py`` writes the record anew from the library as it is."""
import json
import os

import numpy as np

import test_morphology_cpu as M
import test_rank_filter_cpu as R

RECORD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "window_filter_messages.json")

# wrong in two ways at once: what is reported is what is tested first
TWICE = {
    "morphology": [dict(type=ord("f"), size_x=4), dict(type=ord("f"), op=7), dict(op=7, size_x=4), dict(size_x=4, overlap=True), dict(size_y=2, rows=9),
                   dict(rows=9, src=None), dict(op=-1, dst=None)],
    "rank_filter": [dict(type=ord("f"), size_x=4), dict(type=ord("f"), rank=15), dict(size_x=4, rank=225), dict(size_x=4, overlap=True),
                    dict(rank=15, src=None), dict(rank=15, rows=9), dict(rows=9, dst=None)],
}


def label(change):
    return ",".join("%s=%s" % kv for kv in change.items())


def c_answers(lib):
    """{"<entry> <change>": [return value, last error]} for both C entries of both filters"""
    from librir_amd.low_level.misc import last_error

    out = {}
    for name, cases, own in (("morphology", M, "op"), ("rank_filter", R, "rank")):
        cases._bind(lib)
        buf = np.full(2 * 3 * 4 * 5, 7, np.uint16)
        for change in cases.REFUSED + TWICE[name]:
            a = dict(cases.GOOD, src=buf.ctypes.data, dst=buf.ctypes.data + 3 * 4 * 5 * 2)
            a.update({k: v for k, v in change.items() if k != "overlap"})
            if change.get("overlap"):
                a["dst"] = a["src"] + 2 * 4 * 5 * 2  # the last source frame is the first destination frame
            args = (a["type"], a["src"], a["dst"], a["w"], a["h"], a["nframes"], a[own], a["size_x"], a["size_y"], a["rows"])
            for entry, call in (("rir_%s_device" % name, lambda: getattr(lib, "rir_%s_device" % name)(*args, None)),
                                ("rir_%s" % name, lambda: getattr(lib, "rir_%s" % name)(*args))):
                out["%s %s" % (entry, label(change))] = [call(), last_error()]
        assert (buf == 7).all()
    return out


def raised(call):
    try:
        call()
    except Exception as e:  # noqa: BLE001  (the type is what is recorded)
        return [type(e).__name__, str(e)]
    return ["nothing raised", ""]


def python_answers():
    """{"<form> <change>": [exception type, message]} for signal_processing.* and device.*"""
    import torch

    from librir_amd import device as D
    from librir_amd import signal_processing as S

    out = {}
    frames = torch.zeros((6, 4, 5), dtype=torch.uint16)  # (a CPU tensor: the checks come before any device work)
    images = np.zeros((6, 4, 5), np.uint16)
    for name, cases, own, good in (("morphology", M, "op", "open"), ("rank_filter", R, "rank", 4)):
        for change in cases.BAD_PARAMETERS:
            kw = dict({own: good, "size": 3, "rows": None}, **change)
            for form, module, data in (("device", D, frames), ("device, one image", D, frames[0]), ("signal_processing", S, images)):
                out["%s.%s %s" % (form, name, label(change))] = raised(lambda: getattr(module, name)(data, kw[own], kw["size"], kw["rows"]))
        small = torch.zeros((2, 4, 5), dtype=torch.uint16)
        for k, wrong in enumerate((torch.zeros((2, 4, 5), dtype=torch.uint8), torch.zeros((2, 4, 6), dtype=torch.uint16),
                                   torch.zeros((1, 4, 5), dtype=torch.uint16), torch.zeros((2, 4, 5), dtype=torch.uint16))):
            out["device.%s wrong out %d" % (name, k)] = raised(lambda: getattr(D, name)(small, good, 3, out=wrong))
    for k, wrong in enumerate((torch.zeros((2, 4, 5), dtype=torch.uint8), torch.zeros((2, 4, 5), dtype=torch.uint16))):
        out["device.dilate wrong out %d" % k] = raised(lambda: D.dilate(small, 3, out=wrong))
        out["device.window_median wrong out %d" % k] = raised(lambda: D.window_median(small, 3, out=wrong))
    for size in (4, (3, 3, 3), 3.0, 0, (3, -1)):
        out["device.window_median size=%s" % (size,)] = raised(lambda: D.window_median(frames, size))
        out["device.percentile_filter size=%s" % (size,)] = raised(lambda: D.percentile_filter(frames, 25, size))
    return out


def answers(lib):
    return {"c": c_answers(lib), "python": python_answers()}


def test_refusals_are_worded_and_ordered_as_recorded(lib):
    with open(RECORD) as f:
        recorded = json.load(f)
    got = answers(lib)
    for group in ("c", "python"):
        assert sorted(got[group]) == sorted(recorded[group])
        different = {k: (v, recorded[group][k]) for k, v in got[group].items() if v != recorded[group][k]}
        assert not different, different
    assert all(r == -1 for r, _ in got["c"].values())


if __name__ == "__main__":
    from librir_amd.low_level.misc import _lib

    with open(RECORD, "w") as f:
        json.dump(answers(_lib), f, indent=1, sort_keys=True)
        f.write("\n")
