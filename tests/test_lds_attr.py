"""rp::LdsAttr of csrc/row_panel.h - the once-per-device dynamic-LDS attribute of the row-panel kernels' launches - checked without a GPU:
tests/lds_attr_harness.hip includes the header, hands LdsAttr::set_on a made-up device index and a fake attribute call, and checks that a
refused attribute returns -3 with the library's message and is retried at the next launch, that a granted one is set once per device and
kernel, and that device indices outside [0, 64) are served every time.  The program is built with the host sanitizers and run on its own."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_lds_attribute_is_retried_after_failure_and_set_once_after_success(tmp_path):
    from followyourclick_amd import _build
    try:
        hipcc = _build._hipcc()
    except RuntimeError:
        pytest.skip("hipcc not available")
    exe = tmp_path / "lds_attr_harness"
    cmd = [hipcc, *_build._flags("panel_linear.hip"), "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all",
           os.path.join(ROOT, "tests", "lds_attr_harness.hip"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    # the program launches nothing; no device needs to be visible to it
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
