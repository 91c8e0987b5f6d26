"""CPU tests of `framefilt undistort` inside the fused tracker: oat-track-hip's calibration options are checked, with the
reference's texts, before any device is opened; the key-count and exclusion rules of --undistort-key; the C header declares
and oat_amd.ffi binds oatgpu_set_track_undistort."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "build", "bin")
GOLDEN = os.path.join(ROOT, "tests", "golden", "undistort_reference_config.toml")
K9 = "[7473.00,0,408.433,0,8828.00,260.437,0,0,1]"
D5 = "[-0.21,0.07,0.0013,-0.0009,-0.011]"


@pytest.fixture(scope="module")
def track():
    subprocess.check_call(["make", "-s", "-j4", "-C", ROOT, "host"])
    return os.path.join(BIN, "oat-track-hip")


def _run(track, args, sources="oat_tu_a", sinks="oat_tu_p"):
    # (no device is visible: a check that came after opening one would fail with another text)
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    return subprocess.run([track, sources, sinks] + args, capture_output=True, text=True, timeout=30, env=env)


@pytest.mark.parametrize("args,text", [
    (["--camera-matrix", K9], "Required configuration value 'distortion-coeffs' was not specified."),
    (["--distortion-coeffs", D5], "Required configuration value 'camera-matrix' was not specified."),
    (["--camera-matrix", K9, "--distortion-coeffs", "[1,2,3,4]"], "Distortion coefficients consist of 5 to 8 values."),
    (["--camera-matrix", K9, "--distortion-coeffs", "[1,2,3,4,5,6,7,8,9]"], "Distortion coefficients consist of 5 to 8 values."),
    (["--camera-matrix", K9, "--distortion-coeffs", "[0.1,0,0,0,0,0]"], "6 or 7 values"),
    (["--camera-matrix", K9, "--distortion-coeffs", "[0.1,0,0,0,0,0,0]"], "6 or 7 values"),
    (["--camera-matrix", "[7473,0,408,0,8828,260,0,0]", "--distortion-coeffs", D5],
     "'camera-matrix' must be a TOML vector containing 9 elements."),
    (["--camera-matrix", "7473", "--distortion-coeffs", D5], "'camera-matrix' must be a TOML array."),
    (["--camera-matrix", K9, "--distortion-coeffs", D5, "--undistort-key", "undistort"], "mutually exclusive"),
    (["--undistort-key", "undistort"], "give -c FILE KEY"),
])
def test_refusals_before_a_device_is_opened(track, args, text):
    r = _run(track, args)
    assert r.returncode != 0 and text in r.stderr, r.stderr


def test_the_ingest_root_form_checks_the_same(track):
    r = _run(track, ["--ingest-root", "0", "--gpu-index", "0", "--camera-matrix", K9, "--distortion-coeffs", "[1,2,3]"])
    assert r.returncode != 0 and "Distortion coefficients consist of 5 to 8 values." in r.stderr, r.stderr


def test_key_count_is_one_or_one_per_source(track, tmp_path):
    cfg = tmp_path / "cams.toml"
    body = open(GOLDEN).read()
    cfg.write_text("[track]\nerode = 3\n\n" + body + "\n" + body.replace("[undistort]", "[cam1]")
                   .replace("[-53.7430, 20443.3, 0.437918, -0.178999, 51.4270]", "[0.1, 0.0, 0.0, 0.0, 0.0, 0.0]"))
    r = _run(track, ["-c", str(cfg), "track", "--undistort-key", "undistort,undistort,undistort"], "a,b", "p,q")
    assert r.returncode != 0 and "--undistort-key: 3 tables for 2 SOURCEs" in r.stderr, r.stderr
    # two tables for two SOURCEs: every table is read and checked (cam1 holds 6 coefficients) before a device is opened
    r = _run(track, ["-c", str(cfg), "track", "--undistort-key", "undistort,cam1"], "a,b", "p,q")
    assert r.returncode != 0 and "6 or 7 values" in r.stderr, r.stderr
    r = _run(track, ["-c", str(cfg), "track", "--undistort-key", "nothere"], "a,b", "p,q")
    assert r.returncode != 0 and "No configuration table named 'nothere'" in r.stderr, r.stderr
    # the tracker's own table may not hold a calibration besides the named ones ...
    cfg2 = tmp_path / "both.toml"
    cfg2.write_text("[track]\ncamera-matrix = " + K9 + "\ndistortion-coeffs = " + D5 + "\n\n" + body)
    r = _run(track, ["-c", str(cfg2), "track", "--undistort-key", "undistort"])
    assert r.returncode != 0 and "mutually exclusive" in r.stderr, r.stderr


def test_print_partition_is_unchanged_by_a_calibration(track):
    base = _run(track, ["--gpu-index", "0,1", "--print-partition"], "a,b,c", "p,q,r")
    r = _run(track, ["--gpu-index", "0,1", "--print-partition", "--camera-matrix", K9, "--distortion-coeffs", D5], "a,b,c", "p,q,r")
    assert base.returncode == 0 and r.returncode == 0 and r.stdout == base.stdout


def test_usage_names_the_options(track):
    r = subprocess.run([track, "--help"], capture_output=True, text=True, timeout=30)
    for opt in ("--camera-matrix", "--distortion-coeffs", "--undistort-key"):
        assert opt in r.stdout, opt


def test_header_declares_and_ffi_binds_the_entry():
    hdr = open(os.path.join(ROOT, "include", "oatgpu.h")).read()
    assert re.search(r"int\s+oatgpu_set_track_undistort\s*\(\s*oatgpu_ctx\s*\*\s*ctx\s*,\s*int32_t\s+on\s*\)\s*;", hdr)
    assert "#define OATGPU_ABI_VERSION 9" in hdr and "oatgpu_set_track_undistort */" in hdr
    from oat_amd import ffi
    assert "oatgpu_set_track_undistort" in ffi.SIGNATURES
    lib = ffi.load()
    assert lib.oatgpu_set_track_undistort(None, 1) == -1          # a null context is refused, no device needed
