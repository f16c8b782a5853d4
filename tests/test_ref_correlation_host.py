"""not gpu: the recipe that turns the reference's correlation kernel text into the oracle library (oracle/build_ref_correlation.py)
against the reference's own `cupy_kernel` (modules/correlation.py:231-269).  Runs only where a reference checkout is present;
everything is generated under tmp_path, never into the repository."""
import importlib.util
import os
import re
import shutil
import sys
import types

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import ref_harness as rh  # noqa: E402
from oracle import build_ref_correlation as B  # noqa: E402

pytestmark = pytest.mark.skipif(not rh.reference_available(), reason="no reference checkout (CCVS_REFERENCE_ROOT)")

SET_SIZES = re.compile(r"set_sizes\(\d, HIP_SYMBOL\((\w+)_sz\), ([^,]+), ([^,]+), ([^,]+), ([^,]+), st\)")


@pytest.fixture(scope="module")
def ref_module():
    """The reference's correlation.py imported with cupy stubbed (as ref_harness.load_reference does), sys.modules restored."""
    saved = sys.modules.get("cupy")
    cupy = types.ModuleType("cupy")
    cupy.memoize = lambda **kw: (lambda f: f)
    sys.modules["cupy"] = cupy
    try:
        spec = importlib.util.spec_from_file_location("ref_correlation_text", B.reference_source(rh.REF_ROOT))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        if saved is None:
            del sys.modules["cupy"]
        else:
            sys.modules["cupy"] = saved
    return mod


@pytest.fixture(scope="module")
def src():
    return B.read_checked(B.reference_source(rh.REF_ROOT))


def launcher_sizes(n, c, h, w, s):
    """The values the launcher stores in each t_sz, evaluated from its own source."""
    with open(B.LAUNCHER) as f:
        text = f.read()
    env = dict(N=n, C=c, H=h, W=w, s=s, Hp=h + 6 * s, Wp=w + 6 * s, Ho=-(-h // s), Wo=-(-w // s))
    sizes = {m[0]: [eval(e, {}, env) for e in m[1:]] for m in SET_SIZES.findall(text)}
    assert sorted(sizes) == ["input", "output", "rbot0", "top"], sorted(sizes)
    return sizes


@pytest.mark.parametrize("s", (1, 2))
@pytest.mark.parametrize("shape", [(2, 24, 9, 11), (1, 33, 40, 70)], ids=lambda t: "x".join(map(str, t)))
def test_recipe_text_equals_cupy_kernel(ref_module, src, shape, s, tmp_path):
    n, c, h, w = shape
    # the tensors _FunctionCorrelation.forward hands to cupy_kernel (correlation.py:282-330)
    first = torch.empty(n, c, h, w)
    rbot0 = torch.empty(n, h + 6 * s, w + 6 * s, c)
    top = torch.empty(n, 49, -(-h // s), -(-w // s))
    variables = {"kernel_Correlation_rearrange": {"intStride": s, "input": first, "output": rbot0},
                 "kernel_Correlation_updateOutput": {"intStride": s, "rbot0": rbot0, "rbot1": rbot0, "top": top}}
    sizes = launcher_sizes(n, c, h, w, s)
    generated = B.generate_source(src)
    (tmp_path / B.INC_NAME).write_text(generated)
    assert (tmp_path / B.INC_NAME).read_text().count(B.size_macros()) == 1
    assert B.size_macros() == "".join(f"#define SIZE_{k}(t) (t##_sz[{k}])\n" for k in range(4))
    for name, objs in variables.items():
        want = ref_module.cupy_kernel(name, objs)
        text = B.kernel_text(src, name, s)
        assert text in generated
        # what the SIZE_k macros and the launcher's t_sz arrays make of the text at run time
        resolved = B.SIZE_RE.sub(lambda m: str(sizes[m.group(2)][int(m.group(1))]), text)
        for t, tensor in objs.items():   # the launcher's sizes are the tensors' sizes
            if t in sizes:
                assert sizes[t] == list(tensor.shape), (t, sizes[t], tuple(tensor.shape))
        assert f"{name}_s{s}(" in resolved and "{{" not in resolved
        assert resolved.replace(f"{name}_s{s}(", f"{name}(") == want, name


def test_recipe_refuses_other_source(src, tmp_path):
    p = tmp_path / "correlation.py"
    p.write_text(src.replace("total_sum / (float)sumelems", "total_sum / (float)(sumelems + 1)"))
    with pytest.raises(RuntimeError, match="SHA-256"):
        B.read_checked(str(p))


@pytest.mark.skipif(not os.path.exists(B.HIPCC), reason="no hipcc")
def test_generated_source_cross_compiles(src, tmp_path):
    (tmp_path / B.INC_NAME).write_text(B.generate_source(src))
    lib = tmp_path / B.LIB_NAME
    B.compile_library(str(tmp_path), str(lib))
    assert lib.stat().st_size > 0
    if shutil.which("nm"):
        import subprocess
        syms = subprocess.run(["nm", "-D", str(lib)], capture_output=True, text=True).stdout
        assert "ref_correlation7x7" in syms
