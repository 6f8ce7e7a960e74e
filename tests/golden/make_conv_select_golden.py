"""Which kernel does a convolution launch run?  Sweeps the host-side planning helpers of csrc/conv.hip (dy_conv_geometry,
dy_conv_kernel_name, dy_conv_kernel_name_at, dy_conv1x1_kernel_name_live, dy_conv_num_partials, dy_conv_red_supported,
dy_conv_res_supported, dy_conv1x1_segs_supported, dy_conv1x1_segs_kernel_name) and writes every answer to
tests/golden/conv_select.json.gz.  The helpers are arithmetic on the geometry: no GPU is needed, only the built library.

The fixture records what the library of the commit BEFORE the launch-plan refactor of conv.hip answered: it was generated with

    python tests/golden/make_conv_select_golden.py --lib <libdealyolo_hip.so built at that commit> --commit <its hash>

and must not be regenerated from a refactored library to make tests/test_host_conv_select.py pass -- only when a change of the
selection itself is intended and measured.  The commit it was taken at is in the fixture's "meta".

Layout of the fixture: {"meta": ..., "names": [string table], "runs": {tag: {"labels_sha": ..., "vals": [...]}}}.  A run is the whole
sweep under one setting of the environment switches; its values are in sweep order, a kernel name as NAME_BASE + its index into
names and anything else (return codes, geometry numbers, counts) as the plain integer; labels_sha pins the sweep's own case list."""
import argparse
import gzip
import hashlib
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
FIXTURE = os.path.join(HERE, "conv_select.json.gz")
NAME_BASE = 1 << 24  # above every count the helpers return for the swept maps

# (tag, environment, which part of the sweep)
RUNS = (("unset", {}, "all"), ("stream0", {"DY_CONV1X1_STREAM": "0"}, "all"), ("streamforce", {"DY_CONV1X1_STREAM": "force"}, "all"),
        ("fw0", {"DY_CONV_FW": "0"}, "3x3s1"), ("fw80", {"DY_CONV_FW": "80"}, "3x3s1"))

PROBE = r"""
import ctypes as C, json, sys
sys.path[:0] = [%r, %r]
PART = sys.argv[1]
from ultralytics.hip import DY_EPI_ACCUM, DY_EPI_BIAS, DY_EPI_F32OUT, DY_EPI_SILU, DY_EPI_STATS, DY_EPI_STATS_ACC, DySegs, lib
L, buf, out = lib(), C.create_string_buffer(128), []
CH = (3, 6, 8, 16, 24, 32, 48, 64, 72, 80, 88, 96, 128, 144, 160, 192, 256, 264, 320, 384, 512, 1024)
KS = ((1, 1), (3, 1), (3, 2)) if PART == "all" else ((3, 1),)
MAPS = ((1, 20, 20), (64, 40, 40), (3, 48, 48), (64, 80, 80), (16, 160, 160), (1, 320, 320), (2, 27, 45))
EPIS = (0, DY_EPI_ACCUM, DY_EPI_STATS, DY_EPI_STATS | DY_EPI_STATS_ACC, DY_EPI_BIAS | DY_EPI_SILU, DY_EPI_F32OUT | DY_EPI_BIAS)
def name(label, fn, *a):
    buf.value = b""
    rc = fn(*a, buf, 128)
    out.append((label, buf.value.decode() if rc == 0 else rc))
def num(label, v):
    out.append((label, int(v)))
def geometry(cin, cout, ks, st):
    g = [C.c_int(-7) for _ in range(8)]
    rc = L.dy_conv_geometry(cin, cout, ks, st, *[C.byref(v) for v in g])
    num(f"geom/{cin}>{cout}/k{ks}s{st}/rc", rc)
    for i, v in enumerate(g):
        num(f"geom/{cin}>{cout}/k{ks}s{st}/{i}", v.value)
def case(cin, cout, ks, st):
    t = f"{cin}>{cout}/k{ks}s{st}"
    geometry(cin, cout, ks, st)
    name(f"name/{t}", L.dy_conv_kernel_name, cin, cout, ks, st)
    num(f"red/{t}", L.dy_conv_red_supported(cin, cout, ks))
    num(f"res/{t}", L.dy_conv_res_supported(cin, cout, ks, st))
    for n, h, w in MAPS:
        m = f"{t}/{n}x{h}x{w}"
        num(f"partials/{m}/d1", L.dy_conv_num_partials(n, h, w, cin, cout, ks, st, 1))
        wo = (w + 2 * (ks // 2) - ks) // st + 1
        if ks == 3 and st == 1:
            num(f"partials/{m}/d2", L.dy_conv_num_partials(n, h, w, cin, cout, ks, st, 2))
        for e in EPIS:
            name(f"at/{m}/e{e}/d1", L.dy_conv_kernel_name_at, cin, cout, ks, st, wo, 1, e)
            if ks == 3 and st == 1:
                name(f"at/{m}/e{e}/d2", L.dy_conv_kernel_name_at, cin, cout, ks, st, 2 * w, 2, e)
            if ks == 1:
                name(f"live/{m}/e{e}", L.dy_conv1x1_kernel_name_live, cin, cout, n, h, w, e, None, None)
for ks, st in KS:
    for cin in CH:
        for cout in CH:
            case(cin, cout, ks, st)
if PART == "all":
    for cin, cout, st in ((64, 64, 1), (32, 64, 2), (3, 16, 1)):  # an unsupported kernel size: every helper refuses
        case(cin, cout, 5, st)
    # segment tables: channels per member, with and without an up-sampled member (acc bit 1), as the input and as the output
    TABLES = ((16, 16), (32, 32), (64, 64), (16, 32), (32, 64), (64, 32), (64, 16), (16, 16, 16), (32, 32, 32), (64, 64, 64), (64, 32, 32),
              (16, 32, 64), (32, 32, 64), (16, 16, 32), (16, 16, 16, 16), (32, 32, 32, 32), (64, 64, 64, 64), (64, 64, 32, 32), (32, 16, 16, 64),
              (8, 56), (24, 40), (64, 64, 64, 72))
    def table(chs, up, ptr=4096):
        s, c = DySegs(), 0
        s.nseg = len(chs)
        for i, ch in enumerate(chs):
            c += ch
            s.c_end[i], s.ld[i], s.acc[i], s.ptr[i] = c, ch, (2 if up and i == 1 else 0), ptr
        return s, c
    for chs in TABLES:
        for up in (0, 1):
            s, tot = table(chs, up)
            t = "+".join(map(str, chs)) + ("/up" if up else "")
            for other in (32, 64, 128, 48):
                num(f"segs/{t}>{other}/supported", L.dy_conv1x1_segs_supported(tot, other, C.byref(s)))
                name(f"segs/{t}>{other}/name", L.dy_conv1x1_segs_kernel_name, tot, other, C.byref(s))
                for n, h, w in ((1, 40, 40), (64, 80, 80)):
                    for e in (0, DY_EPI_STATS, DY_EPI_STATS | DY_EPI_STATS_ACC, DY_EPI_BIAS | DY_EPI_SILU):
                        name(f"segs/{t}>{other}/live/{n}x{h}x{w}/e{e}", L.dy_conv1x1_kernel_name_live, tot, other, n, h, w, e, C.byref(s), None)
                    for e in (0, DY_EPI_ACCUM):
                        name(f"segs/{other}>{t}/live/{n}x{h}x{w}/e{e}", L.dy_conv1x1_kernel_name_live, other, tot, n, h, w, e, None, C.byref(s))
    for label, (s, tot) in (("null_ptr", table((32, 32), 0, 0)), ("odd_ptr", table((32, 32), 0, 4100))):  # invalid tables
        num(f"segs/{label}/supported", L.dy_conv1x1_segs_supported(tot, 64, C.byref(s)))
        name(f"segs/{label}/name", L.dy_conv1x1_segs_kernel_name, tot, 64, C.byref(s))
        name(f"segs/{label}/live", L.dy_conv1x1_kernel_name_live, tot, 64, 64, 80, 80, 0, C.byref(s), None)
    s, tot = table((32, 32), 0)
    num("segs/wrong_total/supported", L.dy_conv1x1_segs_supported(96, 64, C.byref(s)))
json.dump(out, sys.stdout)
""" % (ROOT, os.path.join(ROOT, "experiment-yolo_amd"))


def sweep(tag, lib_path=None):
    """[(label, value)] of one run of the sweep, probed in a fresh process whose environment carries none of the DY_CONV* / DY_PP*
    switches but the run's own."""
    extra, part = next((e, p) for t, e, p in RUNS if t == tag)
    env = {k: v for k, v in os.environ.items() if not k.startswith(("DY_CONV", "DY_PP"))}
    env.update(extra)
    if lib_path:
        env["DY_HIP_LIB"] = os.path.abspath(lib_path)
    r = subprocess.run([sys.executable, "-c", PROBE, part], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    return [(k, v) for k, v in json.loads(r.stdout[r.stdout.index("[["):])]


def labels_sha(pairs):
    return hashlib.sha256("\n".join(k for k, _ in pairs).encode()).hexdigest()


def load():
    """{tag: [value]} of the fixture with the names decoded, and its meta and per-run label hashes."""
    with gzip.open(FIXTURE, "rt") as f:
        d = json.load(f)
    runs = {t: [d["names"][v - NAME_BASE] if v >= NAME_BASE else v for v in r["vals"]] for t, r in d["runs"].items()}
    return runs, d["meta"], {t: r["labels_sha"] for t, r in d["runs"].items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", required=True, help="libdealyolo_hip.so built at the commit the fixture records")
    ap.add_argument("--commit", required=True, help="hash of that commit")
    a = ap.parse_args()
    names, runs = {}, {}
    for tag, _, _ in RUNS:
        pairs = sweep(tag, a.lib)
        vals = [NAME_BASE + names.setdefault(v, len(names)) if isinstance(v, str) else v for _, v in pairs]
        assert all(isinstance(v, str) or v < NAME_BASE for _, v in pairs)
        runs[tag] = {"labels_sha": labels_sha(pairs), "vals": vals}
        print(tag, len(vals), "entries")
    d = {"meta": {"commit": a.commit, "generator": "tests/golden/make_conv_select_golden.py"}, "names": list(names), "runs": runs}
    with gzip.GzipFile(FIXTURE, "wb", mtime=0) as f:
        f.write(json.dumps(d, separators=(",", ":")).encode())
    print(FIXTURE, os.path.getsize(FIXTURE), "bytes,", len(names), "distinct names")


if __name__ == "__main__":
    main()
