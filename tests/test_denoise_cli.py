"""rtx_render --denoise: argument handling (no GPU: the arguments are judged before a device is opened)"""
import os
import subprocess

import __graft_entry__ as graft

EXE = os.path.join(graft.PKG_DIR, "rtx_render")


def test_denoise_is_refused_with_the_restir_frame():
    graft.load_package()                                   # (raises if the package was never built)
    r = subprocess.run([EXE, "--scene", "cornell", "--denoise", "--mode", "restir"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2, (r.returncode, r.stderr[-500:])
    assert "--denoise" in r.stderr and "restir" in r.stderr
    r = subprocess.run([EXE, "--denoise-levels"], capture_output=True, text=True, timeout=60)      # a value is missing
    assert r.returncode == 2


def test_help_names_the_flag():
    r = subprocess.run([EXE, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0
    for flag in ("--denoise", "--denoise-levels", "--sigma-color", "--sigma-plane", "--adaptive", "--gpus"):
        assert flag in r.stdout, flag
