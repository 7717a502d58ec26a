"""Every compile-time knob the kernel sources keep (rr_kernels.hip, rr_flat_device.h, rr_util.hip,
rr_decode_class.h, rr_snappy.hip) still compiles for gfx950 with a non-default value, so no kept
path rots: a front-end pass (templates instantiated, static_asserts checked) of each variant's device code.
The default build is compiled in full by __graft_entry__.build().  CPU only (hipcc
cross-compiles); skipped where hipcc is absent."""
import os
import re
import shutil
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "redrock_old_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"

# (source, -D flags): one non-default setting per kept knob
VARIANTS = [
    ("rr_kernels.hip", "-DRR_PROBE"),
    ("rr_kernels.hip", "-DRR_ABLATE=1"),
    ("rr_kernels.hip", "-DRR_ABLATE=2"),
    ("rr_kernels.hip", "-DRR_ABLATE=3"),
    ("rr_kernels.hip", "-DRR_ABLATE=4"),
    ("rr_kernels.hip", "-DRR_ABLATE=5"),
    ("rr_kernels.hip", "-DRR_ABLATE=6"),
    ("rr_kernels.hip", "-DRR_ABLATE=7"),
    ("rr_kernels.hip", "-DRR_ABLATE=8"),
    ("rr_kernels.hip", "-DRR_ABLATE=9"),
    ("rr_kernels.hip", "-DRR_ABLATE=10"),
    ("rr_kernels.hip", "-DRR_DEC_W=65536"),
    ("rr_kernels.hip", "-DRR_DEC_SLACK=8192"),
    ("rr_kernels.hip", "-DRR_DEC_NW=4"),
    ("rr_kernels.hip", "-DRR_ZL_VPB=8 -DRR_HH_VPB=16 -DRR_HT_VPB=8 -DRR_LIST_VPB=8"),
    ("rr_kernels.hip", "-DRR_ENC_W=8192 -DRR_ENC_RCAP=256"),
    ("rr_snappy.hip", "-DRR_SNZ_DEC_WIN=16384"),
    ("rr_snappy.hip", "-DRR_SNZ_FRAG=16448"),
    ("rr_snappy.hip", "-DRR_SNZ_K=1"),
    ("rr_snappy.hip", "-DRR_SNZ_K=32"),
    ("rr_snappy.hip", "-DRR_SNZ_SPEC=0"),
    ("rr_snappy.hip", "-DRR_SNZ_SPARSE=4096"),
    ("rr_snappy.hip", "-DRR_SNZ_SPARSE=2048 -DRR_SNZ_K=1"),
    ("rr_snappy.hip", "-DRR_PROBE"),
]


def _knobs(src):
    with open(os.path.join(CSRC, src)) as f:
        text = f.read()
    return set(re.findall(r"^\s*#\s*(?:if|ifdef|ifndef|elif)\b.*?\b(RR_[A-Z0-9_]+)", text, re.M)) - {
        "RR_INTERNAL_H", "RR_KERNELS_H"}


def test_every_knob_has_a_variant():
    """The variant list covers every RR_* knob the sources test (and they stay few)."""
    knobs = set().union(*map(_knobs, ("rr_kernels.hip", "rr_flat_device.h", "rr_util.hip", "rr_decode_class.h",
                                      "rr_snappy.hip")))
    covered = set(re.findall(r"-D(RR_[A-Z0-9_]+)", " ".join(f for _, f in VARIANTS)))
    assert knobs <= covered, sorted(knobs - covered)
    assert len(knobs) <= 16, sorted(knobs)


def _with_headers(src, seen=None):
    """src and the project headers it includes, directly or through one of them."""
    seen = set() if seen is None else seen
    if src not in seen and os.path.exists(os.path.join(CSRC, src)):
        seen.add(src)
        with open(os.path.join(CSRC, src)) as f:
            for inc in re.findall(r'^\s*#\s*include\s+"([^"]+)"', f.read(), re.M):
                _with_headers(os.path.normpath(inc), seen)
    return seen


def _untested(src, flags):
    """The -DRR_X of flags that neither src nor a project header it includes tests in a preprocessor line."""
    tested = set().union(*map(_knobs, _with_headers(src)))
    return set(re.findall(r"-D(RR_[A-Z0-9_]+)", flags)) - tested


def test_every_variant_sets_a_knob_its_source_tests():
    """A variant compiled against a file that never looks at its -D would prove nothing."""
    for src, flags in VARIANTS:
        assert not _untested(src, flags), (src, flags)
    # (the check itself: a variant pointed at the wrong file is found)
    assert _untested("rr_snappy.hip", "-DRR_DEC_W=65536 -DRR_PROBE") == {"RR_DEC_W"}
    assert _untested("rr_kernels.hip", "-DRR_SNZ_K=1") == {"RR_SNZ_K"}
    assert _untested("rr_util.hip", "-DRR_ABLATE=4") == {"RR_ABLATE"}


@pytest.mark.skipif(not os.path.exists(HIPCC) or shutil.which("clang") is None and not os.path.exists(HIPCC),
                    reason="hipcc not installed")
@pytest.mark.parametrize("src,flags", VARIANTS, ids=[f"{s}:{f}" for s, f in VARIANTS])
def test_variant_compiles(src, flags):
    cmd = [HIPCC, "--offload-arch=gfx950", "-std=c++17", "--cuda-device-only", "-fsyntax-only", "-Wno-unused-command-line-argument",
           *flags.split(), src]
    r = subprocess.run(cmd, cwd=CSRC, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
