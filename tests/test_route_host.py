"""The routing rule (eqxvision_amd/csrc/route.h) against the kernels the parent commit chose: tests/data/routes.json holds every
distinct conv / linear entry call of the model zoo's forwards plus rows with every flag the rule reads, recorded on an MI355X from
`mv_last_kernel()`.  tests/route_replay.cpp is a stand-alone host program (no HIP, nothing launched) that answers with the name
route.h gives.  No GPU."""
import json
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "route_replay.cpp")
CXX = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"     # host code only
KERNS = ["generic", "stream1x1", "skinny", "conv3x3c64_v2", "igemm8", "igemm2", "igemm128", "igemm128_oddc"]      # enum class Kern, in order

with open(os.path.join(HERE, "data", "routes.json")) as _f:
    TABLE = json.load(_f)
ROWS = TABLE["rows"]


def _lines():
    out = []
    for entry, args, flags, scratch, _ in ROWS:
        fl = " ".join(f"{k} {v}" for k, v in sorted(flags.items()))
        out.append(f"{entry} {len(args)} {' '.join(map(str, args))} {scratch} {len(flags)} {fl}".rstrip())
    return "\n".join(out) + "\n"


def _build(tmp_path, name, *extra):
    exe = str(tmp_path / name)
    subprocess.run([CXX, "-std=c++17", "-O1", "-Wall", "-Wextra", *extra, SRC, "-o", exe], check=True)
    return exe


def _replay(exe):
    r = subprocess.run([exe], input=_lines(), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    got = [ln.split(" ") for ln in r.stdout.splitlines()]
    assert len(got) == len(ROWS)
    return [("" if g[0] == "-" else g[0], KERNS[int(g[1])], int(g[2])) for g in got]


def _mismatches(got):
    return [(row, g[0]) for row, g in zip(ROWS, got) if g[0] != row[4]]


def test_every_recorded_route_is_reproduced(tmp_path):
    assert len(TABLE["parent"]) == 40 and len(ROWS) > 300
    got = _replay(_build(tmp_path, "route_replay"))
    bad = _mismatches(got)
    assert not bad, f"{len(bad)} of {len(ROWS)} rows differ, first: {bad[:5]}"
    assert len(got) == len(ROWS)                                       # no row skipped
    # the table reaches every kernel family and every tile of the two big GEMM kernels
    own_rule = [g for row, g in zip(ROWS, got) if row[0] != "mv_conv2d_nhwc_grouped64_fwd"]
    assert {g[1] for g in own_rule} == set(KERNS)
    for kern in ("igemm8", "igemm2"):
        assert {g[2] for g in own_rule if g[1] == kern and g[0]} == {1, 2, 3}, kern
    # ... and every flag the rule reads, each override kind and choice
    flags = {k for row in ROWS for k in row[2]}
    assert {"force_generic", "no_stream", "no_stream_narrow", "no_oddc", "no_skinny", "no_igemm8", "no_igemm2", "no_tuned", "no_dual",
            "igemm_tile", "igemm2_tile", "igemm8"} <= flags
    assert {v for row in ROWS for k, v in row[2].items() if k.startswith("ov:")} >= {-1, 1, 2, 3, 7, 8, 9, 10, 11, 12}
    assert any(k.startswith("ovh:") for k in flags) and any(k.startswith("ovd:") for k in flags)


def test_replay_is_clean_under_sanitizers(tmp_path):
    # a stand-alone binary: the snprintf key buffer, the name buffer and the table walk under ASan + UBSan
    exe = _build(tmp_path, "route_replay_san", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    assert not _mismatches(_replay(exe))


def test_table_sees_a_changed_threshold(tmp_path):
    # mutant: igemm8's 256 x 256 tile only from 400 tiles up instead of 150 -- the table must notice
    got = _replay(_build(tmp_path, "route_replay_mutant", "-DMV_ROUTE_T256_MIN=400"))
    bad = _mismatches(got)
    assert bad and all("256x256" in row[4] for row, _ in bad), bad[:3]
