"""The RR_KV_LZ4 route of the batched store I/O (include/rr_kv.h): tests/c/test_kv_lz4.c built and
run the way tests/test_compat.py builds and runs test_kv.c, and the stored streams it samples
decoded by the Python reference (tests/lz4_reference.py) to serObject's bytes.  The harness has no
CPU build (it drives the GPU route), so the run is a GPU test; the build alone runs everywhere."""
import os
import struct
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import lz4_reference as ref  # noqa: E402
from test_compat import write_fixtures  # noqa: E402


def build_kv_lz4(tmp):
    write_fixtures(os.path.join(tmp, "fixtures.h"))
    exe = os.path.join(tmp, "test_kv_lz4")
    cmd = ["gcc", "-std=gnu11", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", tmp,
           os.path.join(ROOT, "tests", "c", "test_kv_lz4.c"), "-L", os.path.join(ROOT, "redrock_old_amd"), "-lrr_serdes",
           "-Wl,-rpath," + os.path.join(ROOT, "redrock_old_amd"), "-o", exe]
    subprocess.run(cmd, check=True)
    return exe


def test_kv_lz4_builds(tmp_path):
    exe = build_kv_lz4(str(tmp_path))
    nm = subprocess.run(["nm", exe], capture_output=True, text=True, check=True).stdout
    assert " U rr_kv_dump_batch" in nm and " U rr_lz4_decompress_batch_host" in nm


@pytest.mark.gpu
def test_kv_lz4_on_gpu(tmp_path):
    """3,000 values dumped (one write batch) and restored with RR_KV_LZ4; the stored bytes decode,
    under the reference rule, to serObject's; a missing key and both flags together are refused."""
    exe = build_kv_lz4(str(tmp_path))
    dump = str(tmp_path / "stored.bin")
    r = subprocess.run([exe, dump], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 failures" in r.stdout
    raw = open(dump, "rb").read()
    p = n = 0
    while p < len(raw):
        (a,) = struct.unpack_from("<I", raw, p)
        stream = raw[p + 4:p + 4 + a]
        p += 4 + a
        (b,) = struct.unpack_from("<I", raw, p)
        canon = raw[p + 4:p + 4 + b]
        p += 4 + b
        st, out, _ = ref.decode(stream)
        assert st == ref.OK and out == canon, (n, ref.STATUS_NAMES[st])
        assert ref.check_encoder_rules(stream) is None
        n += 1
    assert n == 200
