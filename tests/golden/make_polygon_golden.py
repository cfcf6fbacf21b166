"""Generate tests/golden/polygon_maps.npz and polygon_maps_sha256.json from the UNMODIFIED reference C++.

Run in the build container only (needs /root/reference and g++):

    python tests/golden/make_polygon_golden.py

The reference's geometry sources (src/cpp/geometry/*.cpp, with tools/Log.cpp and tools/Misc.cpp on the compile line in place of libtools) are
compiled into a temporary directory, as scripts/wrapper_drop_in_check.py compiles them, and its exported `draw_polygon` is called once per
polygon, in order, on an int32 image filled with the background - on the seeded cases of tests/polygon_cases.py.  Stored: data only - the
maps of the small cases, SHA-256 of the bytes of the 512x640 ones (names ending in _big).  Vertices go in as x + shift (one double addition,
what the device does); a polygon that is out of range in a map (polygon_cases.LIMIT) is not drawn there: the reference leaves it undefined.
"""
import ctypes as ct
import hashlib
import json
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
REF = os.environ.get("RIR_REFERENCE", "/root/reference")

import polygon_cases as PC  # noqa: E402


def build_reference(tmp):
    inc = os.path.join(tmp, "inc")
    os.makedirs(inc)
    text = open(os.path.join(REF, "rir_config.h.in")).read()
    for k, v in (("@PROJECT_NAME@", "librir"), ("@PROJECT_VERSION@", "6.1.2"), ("@PROJECT_VERSION_MAJOR@", "6"),
                 ("@PROJECT_VERSION_MINOR@", "1"), ("@PROJECT_VERSION_PATCH@", "2")):
        text = text.replace(k, v)
    open(os.path.join(inc, "rir_config.h"), "w").write(text)
    g, t = os.path.join(REF, "src", "cpp", "geometry"), os.path.join(REF, "src", "cpp", "tools")
    so = os.path.join(tmp, "libgeometry.so")
    subprocess.check_call(["g++", "-std=c++14", "-O3", "-DNDEBUG", "-fPIC", "-shared", "-DBUILD_GEOMETRY_LIB", "-DBUILD_TOOLS_LIB", "-I" + inc, "-I" + t,
                           "-I" + g, os.path.join(g, "geometry.cpp"), os.path.join(g, "Polygon.cpp"), os.path.join(g, "DrawPolygon.cpp"),
                           os.path.join(t, "Log.cpp"), os.path.join(t, "Misc.cpp"), "-o", so])
    lib = ct.CDLL(so)
    lib.draw_polygon.argtypes = [ct.c_void_p, ct.c_char_p, ct.c_int, ct.c_int, ct.c_void_p, ct.c_int, ct.c_double]
    return lib


def reference_maps(lib, case):
    h, w = case["shape"]
    n = PC.n_maps(case)
    out = np.full((n, h, w), case["background"], np.int32)
    for m in range(n):
        polys = case["sets"][m] if case["per_map"] else case["sets"]
        shift = case["shifts"][m] if case["shifts"] is not None else np.zeros(2)
        for p, poly in enumerate(polys):
            if PC.rounded_vertices(poly, shift) is None:
                continue
            xy = np.ascontiguousarray(poly + shift, np.float64)
            value = p if case["values"] is None else case["values"][p]
            assert lib.draw_polygon(out[m].ctypes.data, b"int32", w, h, xy.ctypes.data, len(xy), float(value)) == 0
    return out


def main():
    tmp = tempfile.mkdtemp(prefix="rir_polygon_")
    try:
        lib = build_reference(tmp)
        arrays, hashes = {}, {}
        for name, case in PC.cases().items():
            maps = reference_maps(lib, case)
            if name.endswith("_big"):
                hashes[name] = hashlib.sha256(maps.tobytes()).hexdigest()
            else:
                arrays[name] = maps
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    np.savez_compressed(os.path.join(HERE, "polygon_maps.npz"), **arrays)
    with open(os.path.join(HERE, "polygon_maps_sha256.json"), "w") as f:
        json.dump(hashes, f, indent=0, sort_keys=True)
        f.write("\n")
    print("polygon maps: %d arrays, %d hashes" % (len(arrays), len(hashes)))


if __name__ == "__main__":
    main()
