"""The encoder kernels' vector-memory stream as compiled for gfx950: resources, and every wait, frame load, store, call and branch of
each kernel in program order, so that the waits in front of the use of a frame can be read off.
    python scripts/packed_ring_isa.py > profiles/packed_ring_isa.txt
    python scripts/packed_ring_isa.py --source other/codec_kernels.hip     # another version of the file, e.g. the parent's
(hipcc -S --cuda-device-only with the library's flags; needs no GPU.)"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from librir_amd.build import COMMON, HIPCC  # noqa: E402

KERNELS = [
    ("rirb1_encode_packed<4, true>", "_ZN3rir19rirb1_encode_packedILi4ELb1EEE"),
    ("rirb1_encode_packed<4, false>", "_ZN3rir19rirb1_encode_packedILi4ELb0EEE"),
    ("rirb1_encode_dense<4>", "_ZN3rir18rirb1_encode_denseILi4EEE"),
    ("rirb1_encode_tiles<true>", "_ZN3rir18rirb1_encode_tilesILb1EEE"),
]
HELPERS = [("staging_flush (out of line)", "_ZN3rir13staging_flush")]
EVENT = re.compile(r"s_waitcnt[^\n]*vmcnt|buffer_load_dwordx4|buffer_store|global_store|global_load|flat_store|flat_load|global_atomic|buffer_load_dwordx2|s_swappc_b64|s_cbranch|s_branch|s_barrier|s_endpgm")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--source", default=os.path.join(ROOT, "librir_amd", "csrc", "codec_kernels.hip"))
    ap.add_argument("--full", action="store_true", help="list every event, not only the summary and the record loops")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "codec.s")
        subprocess.check_call([HIPCC] + COMMON + ["-S", "--cuda-device-only", "-o", out, a.source], stderr=subprocess.DEVNULL)
        lines = open(out).read().split("\n")

    def body(prefix):
        s = next(i for i, l in enumerate(lines) if l.startswith(prefix) and ":" in l)
        e = next(i for i in range(s + 1, len(lines)) if lines[i].startswith(".Lfunc_end"))
        return s, e

    def note(s, e, key):
        for l in lines[e:e + 80]:
            m = re.match(r"; %s\s*[:=]\s*(\d+)" % key, l)
            if m:
                return int(m.group(1))
        return None

    print("codec_kernels.hip for gfx950 (%s): the encoders' waits on the frame ring\n" % " ".join(x for x in COMMON if not x.startswith("-I")))
    for name, prefix in KERNELS + HELPERS:
        try:
            s, e = body(prefix)
        except StopIteration:
            print("%s: not in this version of the file\n" % name)
            continue
        b = lines[s:e]
        ev = [(s + 1 + i, l.strip().split(";")[0].strip()) for i, l in enumerate(b) if l.startswith("\t") and EVENT.search(l)]
        labels = {}
        for i, l in enumerate(b):
            m = re.match(r"(\.LBB\d+_\d+):", l)
            if m:
                labels[m.group(1)] = s + 1 + i
        print("%s" % name)
        print("  codeLenInByte %s, NumVgprs %s, ScratchSize %s" % (note(s, e, "codeLenInByte"), note(s, e, "NumVgprs"), note(s, e, "ScratchSize")))
        loads = [x for x in ev if "buffer_load_dwordx4" in x[1]]
        stores = [x for x in ev if re.search(r"buffer_store|global_store|flat_store", x[1])]
        waits = [x for x in ev if "s_waitcnt" in x[1]]
        print("  frame loads (buffer_load_dwordx4) %d, buffer_store %d, global_store %d, flat_store %d, calls %d" % (
            len(loads), sum("buffer_store" in x[1] for x in stores), sum("global_store" in x[1] for x in stores), sum("flat_store" in x[1] for x in stores),
            sum("swappc" in x[1] for x in ev)))
        hist = {}
        for _, w in waits:
            m = re.search(r"vmcnt\((\d+)\)", w)
            hist[int(m.group(1))] = hist.get(int(m.group(1)), 0) + 1
        print("  waits by count: " + ", ".join("vmcnt(%d) x %d" % (k, hist[k]) for k in sorted(hist)))
        # the compiler names every block's innermost loop in a comment; a loop that holds frame loads is a record loop
        block_of, header, cur = {}, {}, None
        for i, l in enumerate(b):
            m = re.match(r"\.L(BB\d+_\d+):(.*)", l)
            if m:
                cur, note_ = m.group(1), m.group(2)
                for l2 in b[i + 1:i + 4]:  # (the comment goes on in the following lines)
                    if not re.match(r"\s+;", l2):
                        break
                    note_ += l2
                h = re.search(r"in Loop: Header=(BB\d+_\d+)", note_)
                header[cur] = cur if "Inner Loop Header" in note_ else (h.group(1) if h else None)
            block_of[s + 1 + i] = cur
        inner = []
        for hd in sorted({v for k, v in header.items() if v and header.get(v) == v}, key=lambda x: labels[".L" + x]):
            inside = [x for x in ev if header.get(block_of[x[0]]) == hd]
            if any("buffer_load_dwordx4" in x[1] for x in inside):
                inner.append((labels[".L" + hd], inside[-1][0], inside))
        for head, end, inside in inner:
            nl = sum("buffer_load_dwordx4" in x[1] for x in inside)
            ns = sum(bool(re.search(r"buffer_store|global_store|flat_store", x[1])) for x in inside)
            print("  record loop (head at assembly line %d): %d frame loads, %d stores, %d calls; from the head on, in the order of the code:" % (head, nl, ns, sum("swappc" in x[1] for x in inside)))
            seq = []
            for ln, t in inside:
                if "s_waitcnt" in t:
                    seq.append("vmcnt(%s)" % re.search(r"vmcnt\((\d+)\)", t).group(1))
                elif "buffer_load_dwordx4" in t:
                    seq.append("LOAD")
                elif re.search(r"buffer_store|global_store|flat_store", t):
                    seq.append("STORE")
                elif "swappc" in t:
                    seq.append("call")
            print("    " + " ".join(seq))
        in_loops = {x[0] for _, _, ins in inner for x in ins}
        outside = [x for x in ev if "s_waitcnt" in x[1] and x[0] not in in_loops]
        print("  waits outside the record loops: " + " ".join("%d:vmcnt(%s)" % (ln, re.search(r"vmcnt\((\d+)\)", t).group(1)) for ln, t in outside))
        if a.full:
            for ln, t in ev:
                print("    %6d  %s" % (ln, t))
        print()


if __name__ == "__main__":
    main()
