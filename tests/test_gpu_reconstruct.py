"""GPU: grey-level morphological reconstruction, bit for bit against the numpy reference of reconstruct_cases.py (checked against a brute force
of the path definition and against scipy in test_reconstruct_cpu.py).  The kernel converges tiles of 64 x 32 pixels in LDS; the shapes, and the
tile edge each one meets, are listed in reconstruct_cases.py.  Reach (corridors through many tiles, rounds counted), connectivity, extreme
values, the shifted marker's saturation, the rows rule, sentinel fill, batches whose frames converge at different rounds, workspace groups, the
named forms, the host entry, recordings, full-size frames and a cross-check with scipy through label_images."""
import ctypes as ct

import numpy as np
import pytest

from reconstruct_cases import (BORDER, CASES, MARKER, METHODS, SHIFT, TOP, Case, blobs_and_noise, case_id, diagonal, levels_image, make_case, marker_image,
                               reference, serpentine, spiral)

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

TYPE_CHAR = {"uint16": "H", "uint8": "B", "bool": "?"}


def dev(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:
        return torch.from_numpy(a.view(np.int16)).cuda().view(torch.uint16)
    return torch.from_numpy(a).cuda()


def host(t):
    if t.dtype == torch.uint16:
        return t.cpu().view(torch.int16).numpy().view(np.uint16)
    return t.cpu().numpy()


def teq(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(host(a), host(b))


def same(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want)


def entry(mask, marker=None, method="dilation", connectivity=8, mode=MARKER, param=0, output=0, rows=None, out=None, work_bytes=None):
    """rir_reconstruct_device itself, every parameter of the C ABI free; -> (result on the host, rounds)"""
    from librir_amd import device as D

    d_mask = dev(mask)
    d_marker = None if marker is None else dev(marker)
    stack = d_mask if d_mask.dim() == 3 else d_mask.unsqueeze(0)
    n, h, w = stack.shape
    d_out = torch.empty_like(d_mask) if out is None else out
    type_char = ord(TYPE_CHAR[mask.dtype.name])
    need = D._lib.rir_reconstruct_workspace_bytes(type_char, w, h, n) if work_bytes is None else work_bytes
    work = torch.zeros(need // 8 + 1, dtype=torch.int64, device="cuda")
    rounds = ct.c_int(-1)
    r = D._lib.rir_reconstruct_device(type_char, d_mask.data_ptr(), None if d_marker is None else d_marker.data_ptr(), d_out.data_ptr(), w, h, n,
                                      METHODS.index(method), connectivity, mode, param, output, h if rows is None else rows, work.data_ptr(), need,
                                      ct.byref(rounds), D._stream())
    assert r == 0, D.last_error()
    return host(d_out), rounds.value


def corner_marker(mask, value=700):
    marker = np.zeros_like(mask)
    marker[..., 0, 0] = value
    return marker


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_small_cases(case):
    """every type x method x connectivity over three of the nine shapes, the three marker modes in turn, both outputs"""
    mask, marker = make_case(case)
    for output in (0, 1):
        got, rounds = entry(mask, marker, case.method, case.connectivity, case.mode, case.param, output)
        assert same(got, reference(mask, marker, case.method, case.connectivity, case.mode, case.param, output)), output
        assert rounds >= 1


@pytest.mark.parametrize("maker", [serpentine, spiral], ids=["serpentine", "spiral"])
@pytest.mark.parametrize("h,w", [(17, 64), (67, 131)])
def test_reach(maker, h, w):
    """one corridor through the whole image from a marker in one corner (the plain iteration takes 567 and 4 420 steps): all of it fills; on
    3 x 3 tiles that takes more than one round - a tile's halo is read once per round"""
    from librir_amd import device as D

    mask = maker(h, w)
    marker = corner_marker(mask)
    want = np.where(mask > 0, 700, 0).astype(np.uint16)
    assert same(reference(mask, marker), want)
    for connectivity in (8, 4):
        got, rounds = D.reconstruct(dev(marker), dev(mask), connectivity=connectivity, return_rounds=True)
        assert same(host(got), want), connectivity
        assert rounds >= (2 if h > 32 else 1) and rounds <= h * w + 2, rounds
    # the dual: a trench that fills from the corner
    got = D.reconstruct(dev(65535 - marker), dev(65535 - mask), "erosion")
    assert same(host(got), 65535 - want)
    # uint8 and bool run another kernel
    assert same(host(D.reconstruct(dev((marker > 0).astype(np.uint8) * 200), dev((mask > 0).astype(np.uint8) * 250))), (want > 0).astype(np.uint8) * 200)
    assert same(host(D.reconstruct(dev(marker > 0), dev(mask > 0))), want > 0)


@pytest.mark.parametrize("h,w", [(17, 64), (67, 83)])
def test_a_diagonal_corridor_needs_connectivity_8(h, w):
    from librir_amd import device as D

    mask = diagonal(h, w)
    marker = corner_marker(mask)
    assert same(host(D.reconstruct(dev(marker), dev(mask), connectivity=8)), np.where(mask > 0, 700, 0).astype(np.uint16))
    assert same(host(D.reconstruct(dev(marker), dev(mask), connectivity=4)), marker)
    assert same(host(D.reconstruct(dev(marker), dev(mask), connectivity=8)), reference(mask, marker, connectivity=8))


@pytest.mark.parametrize("dtype", ["uint16", "uint8", "bool"])
def test_extreme_values_and_a_marker_above_the_mask(dtype):
    top = TOP[dtype]
    rng = np.random.default_rng(7)
    mask = np.stack([levels_image(rng, 33, 66, dtype, 2) for _ in range(2)])  # 0, the maximum and two levels between
    marker = np.stack([marker_image(rng, m, 0.05) for m in mask])
    above = marker.copy()
    above[:, ::5, ::7] = top  # wherever the mask is lower, the marker is clamped
    flip = lambda a: ~a if a.dtype == np.bool_ else (top - a).astype(a.dtype)  # noqa: E731
    for method in METHODS:
        for seed in (marker, above, np.full_like(mask, top), np.zeros_like(mask)):
            seed = flip(seed) if method == "erosion" else seed
            assert same(entry(mask, seed, method)[0], reference(mask, seed, method)), method
    assert same(entry(mask, mask)[0], mask)  # R(G, G) = G, the marker a stack of its own
    d = dev(mask)
    from librir_amd import device as D

    assert teq(D.reconstruct(d, d), d)  # ... and the mask itself


@pytest.mark.parametrize("dtype", ["uint16", "uint8", "bool"])
def test_the_shifted_marker_saturates(dtype):
    """h above some pixels (G - h saturates at 0, G + h at the maximum), h = the type's maximum and h = 0, both methods and outputs"""
    top = TOP[dtype]
    rng = np.random.default_rng(11)
    mask = np.stack([levels_image(rng, 33, 66, dtype), levels_image(rng, 33, 66, dtype, 40)])
    for method in METHODS:
        for param in sorted({0, 1, top // 3, top - 1, top}):
            for output in (0, 1):
                got = entry(mask, None, method, 8, SHIFT, param, output)[0]
                assert same(got, reference(mask, None, method, 8, SHIFT, param, output)), (method, param, output)
                if param == 0:
                    assert same(got, mask if output == 0 else np.zeros_like(mask))


@pytest.mark.parametrize("case", [c for c in CASES if c.h >= 17][::3], ids=case_id)
def test_rows(case):
    """the last three rows, every row and all but one row outside the image: copied from the MASK, read by nothing - the border marker uses
    row rows - 1"""
    mask, marker = make_case(case)
    for rows in (case.h - 3, 0, 1):
        for output in (0, 1):
            got = entry(mask, marker, case.method, case.connectivity, case.mode, case.param, output, rows=rows)[0]
            assert same(got, reference(mask, marker, case.method, case.connectivity, case.mode, case.param, output, rows)), (rows, output)
            assert same(got[:, rows:], mask[:, rows:])


def test_the_border_marker_uses_the_last_image_row():
    mask = np.zeros((1, 33, 66), np.uint16)
    mask[0, 20:30, 10:20] = 500  # a block that touches row 29 = rows - 1 when rows is 30, and nothing when all rows count
    assert same(entry(mask, None, "dilation", 8, BORDER, 0, 1)[0], mask)  # clear_border keeps it
    cleared = entry(mask, None, "dilation", 8, BORDER, 0, 1, rows=30)[0]
    assert not cleared[0, :30].any() and same(cleared[0, 30:], mask[0, 30:])
    assert same(cleared, reference(mask, None, "dilation", 8, BORDER, 0, 1, 30))


@pytest.mark.parametrize("case", [CASES[1], CASES[8], CASES[13], CASES[22], CASES[27], CASES[35]], ids=case_id)
def test_out_is_fully_overwritten(case):
    from librir_amd import device as D

    mask, marker = make_case(case)
    for rows in (case.h, max(0, case.h - 3)):
        for output in (0, 1):
            want = reference(mask, marker, case.method, case.connectivity, case.mode, case.param, output, rows)
            for sentinel in (0, 1):  # (no value is free in a bool image: two fills, one of which every pixel differs from)
                fill = np.full(mask.shape, 165 if sentinel and mask.dtype != np.bool_ else sentinel).astype(mask.dtype)
                out = dev(fill)
                got = entry(mask, marker, case.method, case.connectivity, case.mode, case.param, output, rows=rows, out=out)[0]
                assert same(got, want), (rows, output, sentinel)
    d = dev(mask)
    out = torch.empty_like(d)
    assert D.fill_holes(d, out=out) is out and D.h_dome(d, 1 if case.dtype == "bool" else 9, out=out) is out


def mixed_batch():
    """frames that converge at different rounds in one stack: constant frames (the marker the mask itself, or nothing to fill: one round), noise (a few), a serpentine through 3 x 3 tiles (many)"""
    rng = np.random.default_rng(21)
    h, w = 67, 131
    mask = np.stack([np.full((h, w), 900, np.uint16), serpentine(h, w), rng.integers(0, 65536, (h, w)).astype(np.uint16), np.zeros((h, w), np.uint16),
                     spiral(h, w), levels_image(rng, h, w, "uint16")])
    marker = np.stack([mask[0], corner_marker(mask[1]), marker_image(rng, mask[2]), corner_marker(mask[3]), corner_marker(mask[4]),
                       marker_image(rng, mask[5])])
    return mask, marker


def test_a_batch_equals_its_frames():
    mask, marker = mixed_batch()
    whole, rounds = entry(mask, marker)
    assert same(whole, reference(mask, marker))
    each = [entry(mask[i], marker[i]) for i in range(len(mask))]
    for i, (got, _) in enumerate(each):
        assert got.shape == mask[i].shape and np.array_equal(whole[i], got), i
    took = [r for _, r in each]
    assert rounds >= 2 and took[0] == 1 and took[1] >= 2 and took[3] == 1 and took[4] >= 2, (rounds, took)


def test_workspace_groups_give_the_same_bits():
    """a workspace of one frame's share: groups of one frame; of two frames' share and a bit: groups of two"""
    from librir_amd import device as D

    mask, marker = mixed_batch()
    whole = entry(mask, marker)[0]
    one = D._lib.rir_reconstruct_workspace_bytes(ord("H"), mask.shape[2], mask.shape[1], 1)
    assert D._lib.rir_reconstruct_workspace_bytes(ord("H"), mask.shape[2], mask.shape[1], len(mask)) == len(mask) * one
    for size in (one, 2 * one + 8):
        assert same(entry(mask, marker, work_bytes=size)[0], whole), size
        assert same(entry(mask, None, "erosion", 4, BORDER, 0, 1, rows=60, work_bytes=size)[0], reference(mask, None, "erosion", 4, BORDER, 0, 1, 60))


def test_named_forms_equal_the_generic_one():
    from librir_amd import device as D

    rng = np.random.default_rng(31)
    for dtype, hh in (("uint16", 4000), ("uint8", 30), ("bool", 1)):
        mask = np.stack([levels_image(rng, 33, 83, dtype, 12) for _ in range(2)])
        d = dev(mask)
        forms = [(D.h_maxima, (hh,), ("dilation", SHIFT, hh, 0)), (D.h_dome, (hh,), ("dilation", SHIFT, hh, 1)), (D.h_minima, (hh,), ("erosion", SHIFT, hh, 0)),
                 (D.h_basin, (hh,), ("erosion", SHIFT, hh, 1)), (D.fill_holes, (), ("erosion", BORDER, 0, 0)), (D.clear_border, (), ("dilation", BORDER, 0, 1))]
        for f, own, (method, mode, param, output) in forms:
            for connectivity, rows in ((8, None), (4, 30)):
                want = reference(mask, None, method, connectivity, mode, param, output, rows)
                assert same(host(f(d, *own, connectivity=connectivity, rows=rows)), want), (f.__name__, connectivity)
                assert same(host(f(d[0], *own, connectivity, rows)), want[0])
                out = torch.empty_like(d)
                assert f(d, *own, connectivity, rows, out=out) is out and same(host(out), want)
        for connectivity, rows in ((8, None), (4, 30)):
            top_rows = slice(None) if rows is None else slice(0, rows)
            for f, method in ((D.regional_maxima, "dilation"), (D.regional_minima, "erosion")):
                want = np.zeros(mask.shape, bool)
                want[:, top_rows] = reference(mask, None, method, connectivity, SHIFT, 1, 1, rows)[:, top_rows] != 0
                got = f(d, connectivity, rows)
                assert got.dtype == torch.bool and same(host(got), want), (f.__name__, connectivity)
                out = torch.empty(mask.shape, dtype=torch.bool, device="cuda")
                assert f(d, connectivity, rows, out=out) is out and same(host(out), want)
        marker = np.stack([marker_image(rng, m) for m in mask])
        got, rounds = D.reconstruct(dev(marker), d, "dilation", 4, 30, return_rounds=True)
        assert same(host(got), reference(mask, marker, "dilation", 4, rows=30)) and rounds >= 1
    # a plateau of value 0 is no maximum, one of the type's maximum no minimum
    flat = torch.zeros((1, 17, 64), dtype=torch.uint16, device="cuda")
    assert not D.regional_maxima(flat).any() and D.regional_minima(flat).all()
    assert D.regional_maxima(dev(np.full((17, 64), 5, np.uint16))).all() and not D.regional_minima(dev(np.full((17, 64), 65535, np.uint16))).any()


def test_overlap_is_refused():
    from librir_amd import device as D

    d = dev(make_case(Case("uint16", 17, 64, 4, "dilation", 8, SHIFT, 0, 1))[0])
    with pytest.raises(RuntimeError, match="overlap"):
        D.h_dome(d[:3], 5, out=d[1:])
    with pytest.raises(RuntimeError, match="overlap"):
        D.reconstruct(d[:2], d[2:], out=d[1:3])


@pytest.mark.parametrize("dtype", ["uint16", "uint8", "bool"])
def test_host_entry_equals_device_entry(dtype):
    from librir_amd import signal_processing as S

    rng = np.random.default_rng(41)
    hh = {"uint16": 3000, "uint8": 20, "bool": 1}[dtype]
    for (n, h, w), connectivity, rows in [((5, 67, 83), 8, None), ((3, 17, 64), 4, 14), ((2, 1, 1), 8, None), ((1, 3, 5), 4, 0)]:
        mask = np.stack([levels_image(rng, h, w, dtype, 12) for _ in range(n)])
        marker = np.stack([marker_image(rng, m) for m in mask])
        for method in METHODS:
            want = entry(mask, marker, method, connectivity, rows=rows)[0]
            assert same(want, reference(mask, marker, method, connectivity, rows=rows))
            assert same(S.reconstruct(marker, mask, method, connectivity, rows), want)
            assert same(S.reconstruct(marker[0], mask[0], method, connectivity, rows), want[0])
        assert same(S.h_maxima(mask, hh, connectivity, rows), reference(mask, None, "dilation", connectivity, SHIFT, hh, 0, rows))
        assert same(S.h_dome(mask, hh, connectivity, rows), reference(mask, None, "dilation", connectivity, SHIFT, hh, 1, rows))
        assert same(S.fill_holes(mask, connectivity, rows), reference(mask, None, "erosion", connectivity, BORDER, 0, 0, rows))


def test_host_entry_in_slabs():
    """more than one 64 MiB slab of frames: 110 frames of 640 x 512 uint16 (uniform noise: the plain iteration takes 6 steps)"""
    from librir_amd import signal_processing as S

    rng = np.random.default_rng(9)
    stack = np.tile(rng.integers(0, 65536, (5, 512, 640)).astype(np.uint16), (22, 1, 1))
    got = S.h_dome(stack, 3000)
    want = reference(stack[:5], None, "dilation", 8, SHIFT, 3000, 1)
    assert same(got[:5], want) and np.array_equal(got[5:], np.tile(want, (21, 1, 1)))


def record(path, frames):
    from librir_amd.video_io import IRSaver

    n, h, w = frames.shape
    with IRSaver(str(path), w, h, h) as s:
        for i in range(n):
            s.add_image(frames[i], i * 20000000 + 7)
    return str(path)


def test_recordings(tmp_path):
    from librir_amd import device as D
    from librir_amd.synthetic import s1_noisy_background
    from librir_amd.video_io import IRMovie

    n, h, w = 7, 67, 83
    arr = s1_noisy_background(n, h, w, seed=4)
    with IRMovie.from_filename(record(tmp_path / "m.h264", arr)) as mov:
        for sel, hh, connectivity, rows in [(slice(None), 40, 8, None), (slice(1, None, 2), 300, 4, h - 3), (3, 7, 8, None), (slice(0, 0), 40, 8, None)]:
            frames = mov.to_tensor(sel)
            for form, dform, output in ((mov.h_dome, D.h_dome, 1), (mov.h_maxima, D.h_maxima, 0)):
                want = dform(frames, hh, connectivity, rows)
                got = form(hh, sel, connectivity, rows)
                assert got.dtype == torch.uint16 and got.shape == frames.shape and teq(got, want), (sel, output)
                out = dev(np.full(tuple(want.shape), 12345, np.uint16))
                assert form(hh, selection=sel, connectivity=connectivity, rows=rows, out=out) is out and teq(out, want)
                assert same(host(got), reference(host(frames), None, "dilation", connectivity, SHIFT, hh, output, rows))
        # pieces smaller than the selection give the same bits
        want = mov.h_dome(40)
        mov._STATS_PIECE_BYTES = 3 * h * w * 2
        assert teq(mov.h_dome(40), want)
        with pytest.raises(ValueError):
            mov.h_dome(70000)
        with pytest.raises(ValueError):
            mov.h_maxima(40, connectivity=6)
        with pytest.raises(RuntimeError):
            mov.h_dome(40, out=torch.empty((n, h, w + 1), dtype=torch.uint16, device="cuda"))


def test_full_size_frames():
    """two 512 x 640 frames of smooth blobs plus noise, h_dome at h = 50 (the plain iteration takes about a hundred steps), and one of uniform
    noise at h = 3 000 (six steps)"""
    from librir_amd import device as D

    blobs = np.stack([blobs_and_noise(seed=1), blobs_and_noise(seed=2)])
    its = []
    want = reference(blobs, None, "dilation", 8, SHIFT, 50, 1, iterations=its)
    assert min(its) > 50
    assert same(host(D.h_dome(dev(blobs), 50)), want)
    noise = np.random.default_rng(1).integers(0, 65536, (1, 512, 640)).astype(np.uint16)
    assert same(host(D.h_dome(dev(noise), 3000)), reference(noise, None, "dilation", 8, SHIFT, 3000, 1))


def test_clear_border_and_fill_holes_agree_with_the_scipy_route():
    """bool masks through clear_border / fill_holes and label_images against scipy's label of binary_fill_holes / of the components that do
    not touch the border"""
    ndi = pytest.importorskip("scipy.ndimage")
    from librir_amd import device as D

    rng = np.random.default_rng(51)
    masks = ndi.binary_opening(rng.random((3, 67, 130)) < 0.6, np.ones((1, 2, 2), bool))
    filled = host(D.fill_holes(dev(masks)))
    assert same(filled, np.stack([ndi.binary_fill_holes(m) for m in masks]))
    kept = host(D.clear_border(dev(masks), connectivity=8))
    eight = np.ones((3, 3), bool)
    want = np.zeros_like(masks)
    for i, m in enumerate(masks):
        lab, k = ndi.label(m, eight)
        edge = np.unique(np.concatenate([lab[0], lab[-1], lab[:, 0], lab[:, -1]]))
        want[i] = m & ~np.isin(lab, edge[edge > 0])
    assert same(kept, want) and want.any() and (want != masks).any()
    for ours, theirs in ((filled, filled), (kept, want)):
        labels, counts = D.label_images(dev(ours))[0], [ndi.label(m)[1] for m in theirs]  # (label_images joins along the cross)
        got = host(labels)
        assert [len(np.unique(g[g > 0])) for g in got] == counts
        assert same(got > 0, theirs)
