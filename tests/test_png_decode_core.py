"""not gpu: the inflate of the PNG decoder (ccvs_amd/csrc/png_decode_core.h) as host code under
AddressSanitizer and UndefinedBehaviorSanitizer.  tests/png_decode_core_check.cpp, a program of its own, is built here with
-fsanitize=address,undefined and run as a child process on a file of cases this test writes:

  1. the plain streams of tests/png_decode_ref.py (zlib's at every level and strategy, the planted buffer, the encoder mirror's, stored
     and wbits = 9 streams) and the hand-assembled ones: the status and, with status 0, the bytes of the spec mirror;
  2. its 2000 deterministic mutations -- truncation, one byte altered, a random tail, a wrong expected size: the sanitizers report
     nothing, the guards around the output stay whole, the status is the mirror's word and with status 0 the bytes are the mirror's.
"""
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import png_decode_ref as D  # noqa: E402


def blob(stream, expect, status, out):
    head = np.array([len(stream), expect, status, int(status == 0)], dtype=np.int64)
    return head.tobytes() + stream + (out if status == 0 else b"")


def test_inflate_core_under_sanitizers(tmp_path):
    cases = D.judged("plain") + D.judged("hand") + D.judged("mutations")
    assert len(D.judged("mutations")) == 2000
    clean = sum(st == 0 for _, _, _, st, _ in cases)
    exe = str(tmp_path / "core_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                    "-I", os.path.join(ROOT, "ccvs_amd", "csrc"), os.path.join(HERE, "png_decode_core_check.cpp"), "-o", exe], check=True)
    (tmp_path / "cases.bin").write_bytes(b"".join(blob(s, e, st, out) for _, s, e, st, out in cases))
    run = subprocess.run([exe, str(tmp_path / "cases.bin")], capture_output=True, text=True)
    print(run.stdout, run.stderr[-4000:])
    assert run.returncode == 0, (run.returncode, run.stderr[-2000:])
    assert run.stdout.split() == ["cases", str(len(cases)), "clean", str(clean), "failed", str(len(cases) - clean), "wrong", "0"]
