"""not gpu: the entropy decoder of the JPEG decoder (ccvs_amd/csrc/jpeg_decode_core.h) as host code under
AddressSanitizer and UndefinedBehaviorSanitizer.  tests/jpeg_decode_core_check.cpp, a program of its own, is built here with
-fsanitize=address,undefined and run as a child process on a file of cases this test writes:

  1. every unit of three fixture files (4:2:0 and 4:4:4 with restart intervals; 4:2:2 with the file's own optimised Huffman tables):
     status 0 and the coefficients the spec mirror tests/jpeg_decode_ref.py decodes;
  2. 360 deterministic mutations of those units -- truncations, one byte altered, a tail of random bytes, an MCU count the bytes do not
     serve: the sanitizers report nothing, the guards around the coefficients and every block outside the unit's own MCUs stay as they
     were, the status is zero exactly where the mirror's is, and with status 0 the coefficients are the mirror's.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import jpeg_decode_ref as D  # noqa: E402

FILES = ("noise_17x35/q100/s2/r3", "smooth_31x50/q30/s1/opt", "noise_16x40_r3/q100/s0/r3")


def case(data, p, record, first, count):
    """One case of the check program, the verdict and the coefficients being the mirror's."""
    coef = D.empty_coefficients(p)
    status = D.decode_unit(data, p, first, count, coef)
    hs, vs, mcux, mcuy = D.geometry(p["h"], p["w"], p["sampling"])
    head = np.array([hs, vs, mcux, mcuy, first, count, len(data), int(status != 0), int(status == 0)], dtype=np.int64)
    want = np.concatenate([c.reshape(-1) for c in coef]).astype(np.int16).tobytes() if status == 0 else b""
    return head.tobytes() + record + bytes(data) + want, status


def build_cases(fixture):
    from ccvs_amd.tools import mjpeg
    rng = np.random.RandomState(7)
    plain, mutated, statuses = [], [], []
    for key in FILES:
        data = fixture[key][0]
        p = D.parse(data)
        record = mjpeg.decode_tables(mjpeg.parse_jpeg(data))
        hs, vs, mcux, mcuy = D.geometry(p["h"], p["w"], p["sampling"])
        units = D.split_units(p["scan"], p["ri"], mcux * mcuy)
        for off, length, first, count in units:
            blob, status = case(p["scan"][off:off + length], p, record, first, count)
            assert status == 0, (key, first)
            plain.append(blob)
        for i in range(120):
            off, length, first, count = units[rng.randint(len(units))]
            unit = bytearray(p["scan"][off:off + length])
            kind = i % 4
            if kind == 0:
                unit = unit[:rng.randint(0, length)]                                         # truncated
            elif kind == 1:
                unit[rng.randint(length)] ^= rng.randint(1, 256)                             # one byte altered
            elif kind == 2:
                cut = rng.randint(0, length)
                unit[cut:] = rng.randint(0, 256, size=length - cut).astype(np.uint8).tobytes()    # a tail of random bytes
            else:
                first, count = (first, count - 1) if count > 1 and i % 8 == 3 else (0, mcux * mcuy)   # fewer / more MCUs than the bytes hold
            blob, status = case(bytes(unit), p, record, first, count)
            mutated.append(blob)
            statuses.append(status)
    return plain, mutated, statuses


def test_entropy_core_under_sanitizers(tmp_path, golden_dir):
    fixture, _ = D.load_fixture(os.path.join(golden_dir, "mjpeg_decode_cases.npz"))
    plain, mutated, statuses = build_cases(fixture)
    assert len(mutated) == 360 and len(plain) >= 5
    seen = {s: statuses.count(s) for s in sorted(set(statuses))}
    print("mirror's statuses over the mutations:", seen)
    assert seen.get(D.OK, 0) >= 5 and seen.get(D.BAD_CODE, 0) + seen.get(D.BAD_INDEX, 0) >= 5 and seen.get(D.OVERRUN, 0) >= 5 and seen.get(D.LEFTOVER, 0) >= 5
    exe = str(tmp_path / "core_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                    "-I", os.path.join(ROOT, "ccvs_amd", "csrc"), os.path.join(HERE, "jpeg_decode_core_check.cpp"), "-o", exe], check=True)
    (tmp_path / "cases.bin").write_bytes(b"".join(plain + mutated))
    run = subprocess.run([exe, str(tmp_path / "cases.bin")], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0, (run.returncode, run.stderr[-2000:])
    assert run.stdout.split() == ["cases", str(len(plain) + 360), "clean", str(len(plain) + seen[D.OK]), "failed", str(360 - seen[D.OK]), "wrong", "0"]
