"""The SAVE request of the snapshot pipes (RR_RDB_SAVE_TAG, include/rr_rdb.h; the child side
rr_rdbsave_request, include/rr_rdbsave.h): tests/c/test_rdbsave_pipe.c over real pipes and an
in-memory store of the golden fixtures."""
import os
import subprocess

import pytest

from helpers import golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _c_bytes(b):
    return "{" + ",".join(str(x) for x in b) + "}" if b else "{0}"


def write_fixtures(path):
    g = golden()
    fx = g["kats"] + g["edges"]
    lines = ["typedef struct { const char *name; const unsigned char *blob; size_t len; int status; } fixture_t;"]
    for i, f in enumerate(fx):
        lines.append(f"static const unsigned char B{i}[] = {_c_bytes(bytes.fromhex(f['blob']))};")
    lines.append(f"#define N_FIXTURES {len(fx)}")
    lines.append("static const fixture_t FIXTURES[N_FIXTURES] = {")
    for i, f in enumerate(fx):
        lines.append(f'  {{"{f["name"]}", B{i}, {len(bytes.fromhex(f["blob"]))}, {f["value"].get("status", 0)}}},')
    lines.append("};")
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")


def build(tmp):
    write_fixtures(os.path.join(tmp, "fixtures.h"))
    exe = os.path.join(tmp, "test_rdbsave_pipe")
    lib = os.path.join(ROOT, "redrock_old_amd")
    subprocess.run(["gcc", "-std=gnu11", "-O2", "-Wall", "-Werror", "-pthread", "-I", os.path.join(ROOT, "include"),
                    "-I", tmp, os.path.join(ROOT, "tests", "c", "test_rdbsave_pipe.c"), "-L", lib, "-lrr_serdes",
                    "-Wl,-rpath," + lib, "-o", exe], check=True)
    return exe


def test_rdbsave_pipe_program_builds(tmp_path):
    nm = subprocess.run(["nm", build(str(tmp_path))], capture_output=True, text=True, check=True).stdout
    assert "rr_rdbsave_request" in nm and "rr_rdb_serve" in nm


def test_rdbsave_pipe_bench_builds(tmp_path):
    """tests/c/bench_rdbsave_pipe.c (the keys/s of RAW, FLAT and SAVE in DESIGN.md section 11) compiles and links."""
    exe = str(tmp_path / "bench_rdbsave_pipe")
    lib = os.path.join(ROOT, "redrock_old_amd")
    subprocess.run(["gcc", "-std=gnu11", "-O2", "-Wall", "-Werror", "-pthread", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "c", "bench_rdbsave_pipe.c"), "-L", lib, "-lrr_serdes",
                    "-Wl,-rpath," + lib, "-o", exe], check=True)
    assert os.path.exists(exe)


@pytest.mark.gpu
def test_rdbsave_pipe_on_gpu(tmp_path):
    r = subprocess.run([build(str(tmp_path))], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 failures" in r.stdout
