"""not gpu: the host side of LPIPS from user-supplied weights.

  1. the float64 mirror tests/lpips_ref.py against an independently built nn.Sequential in torchvision's layout, tapped by module index
     3 / 8 / 15 / 22 / 29 (this pins the layer numbering); mirror(x, x) == 0; a hand-computed one-position case of the channel
     normalisation and the weighted distance, the all-zero vector included; the random weights keep the activations O(1) and give
     scores near 0.1 for y = clamp(x + 0.1 randn);
  2. `load_lpips_weights` on each format it accepts, and on a missing key, a wrong shape and four heads; the converter's round trip;
  3. `lib.LPIPS_EXPORTS` equals what include/ccvs_hip_lpips.h declares, the built library exports it, the lists are disjoint, bad
     arguments are refused before any launch;
  4. `--lpips_weights` parses; without weights `get_lpips` raises and `print_scores([None], ...)` prints the line there was.
"""
import ctypes
import os
import re
import subprocess
import sys

import pytest
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import lpips_ref as R  # noqa: E402


@pytest.fixture(scope="module")
def weights():
    return R.random_weights(11)


@pytest.fixture
def M():
    from ccvs_amd.tools.pytorch_metrics import metrics
    metrics.set_lpips_weights(None)
    yield metrics
    metrics.set_lpips_weights(None)


# ------------------------------------------------------------------ 1: the mirror
def _torchvision_layout(weights):
    """vgg16().features as torchvision builds it (make_layers over configuration 'D'), written out here without the mirror's tables."""
    layers, cin = [], 3
    for v in [64, 64, "M", 128, 128, "M", 256, 256, 256, "M", 512, 512, 512, "M", 512, 512, 512, "M"]:
        if v == "M":
            layers.append(nn.MaxPool2d(kernel_size=2, stride=2))
        else:
            layers += [nn.Conv2d(cin, v, kernel_size=3, padding=1), nn.ReLU(inplace=False)]
            cin = v
    net = nn.Sequential(*layers)
    assert len(net) == 31
    net.load_state_dict({k[len("features."):]: v for k, v in weights["vgg"].items()})
    return net.eval()


def test_mirror_matches_a_sequential_tapped_by_module_index(weights):
    x, y = R.pair((2, 3, 37, 45), 3)
    net = _torchvision_layout(weights)
    mean, std = torch.tensor(R.MEAN).view(1, 3, 1, 1), torch.tensor(R.STD).view(1, 3, 1, 1)

    def taps(img):
        h, out = (img - mean) / std, []
        for i, mod in enumerate(net):
            h = mod(h)
            if i in (3, 8, 15, 22, 29):
                out.append(h)
        return out

    with torch.no_grad():
        fx, fy = taps(x), taps(y)
        assert [t.shape[1] for t in fx] == [64, 128, 256, 512, 512] and fx[4].shape[2:] == (2, 2)
        mine = R.features(x, weights, torch.float32)
        for a, b in zip(fx, mine):
            assert a.shape == b.shape and (a - b).abs().max() <= 1e-5 * a.abs().max()
            assert 0.05 < a.abs().mean() < 20, "the random weights keep the activations O(1)"
        total = torch.zeros(2)
        for a, b, w in zip(fx, fy, weights["lin"]):
            na = a / (torch.sqrt((a ** 2).sum(1, keepdim=True)) + 1e-10)
            nb = b / (torch.sqrt((b ** 2).sum(1, keepdim=True)) + 1e-10)
            total += (w * (na - nb) ** 2).sum(1, keepdim=True).mean(dim=(2, 3)).view(-1)
    want = R.per_image(x, y, weights)
    assert want.dtype == torch.float64 and ((total.double() - want).abs() / want).max() < 1e-5
    assert ((R.per_image(x, y, weights, torch.float32).double() - want).abs() / want).max() < 5e-6
    assert 0.02 < want.min() and want.max() < 0.5, want     # near 0.1 per image for 0.1 randn of noise
    assert abs(R.lpips(x, y, weights).item() - want.mean().item()) < 1e-15


def test_mirror_of_equal_images_is_zero(weights):
    x, _ = R.pair((2, 3, 32, 32), 4)
    assert torch.equal(R.per_image(x, x.clone(), weights), torch.zeros(2, dtype=torch.float64))


def test_one_position_by_hand():
    # a = (3, 4), b = (0, 5): a / 5 = (0.6, 0.8), b / 5 = (0, 1); w = (2, 0.5): 2 * 0.36 + 0.5 * 0.04 = 0.74
    a = torch.tensor([3.0, 4.0], dtype=torch.float64).view(1, 2, 1, 1)
    b = torch.tensor([0.0, 5.0], dtype=torch.float64).view(1, 2, 1, 1)
    w = torch.tensor([2.0, 0.5]).view(1, 2, 1, 1)
    assert abs(R.layer_distance(a, b, w).item() - 0.74) < 1e-9     # (the 1e-10 in the denominators moves the ninth digit)
    # the all-zero vector: 0 / (0 + 1e-10) = 0, so the distance is sum w a_hat^2 = 2 * 0.36 + 0.5 * 0.64 = 1.04, not NaN
    z = torch.zeros_like(a)
    assert abs(R.layer_distance(a, z, w).item() - 1.04) < 1e-9
    assert R.layer_distance(z, z, w).item() == 0.0


# ------------------------------------------------------------------ 2: the loader and the converter
def test_loader_formats(weights, tmp_path):
    from ccvs_amd.tools.pytorch_metrics.lpips import load_lpips_weights, VGG16_CONVS, LIN_CHANNELS
    assert [n for n, _, _ in VGG16_CONVS] == [0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28] and LIN_CHANNELS == (64, 128, 256, 512, 512)
    same = lambda got: (all(torch.equal(got["vgg"][k], weights["vgg"][k]) for k in weights["vgg"]) and len(got["vgg"]) == 26
                        and all(torch.equal(a, b) and a.shape == (1, b.shape[1], 1, 1) for a, b in zip(got["lin"], weights["lin"])) and len(got["lin"]) == 5)
    assert same(load_lpips_weights(weights))
    bare = {k[len("features."):]: v for k, v in weights["vgg"].items()}
    bare["classifier.0.weight"] = torch.zeros(3, 3)      # ignored
    flat = [t.reshape(-1) for t in weights["lin"]]
    assert same(load_lpips_weights({"vgg": bare, "lin": flat}))
    named = {f"lin{i}.model.1.weight": t for i, t in enumerate(weights["lin"])}
    assert same(load_lpips_weights({"vgg": weights["vgg"], "lin": dict(reversed(list(named.items())))}))
    assert same(load_lpips_weights({"vgg": weights["vgg"], "lin": tuple(weights["lin"])}))
    path = tmp_path / "w.pt"
    torch.save({"vgg": weights["vgg"], "lin": named}, path)
    assert same(load_lpips_weights(str(path))) and same(load_lpips_weights(path))
    half = {k: v.double() for k, v in weights["vgg"].items()}
    assert load_lpips_weights({"vgg": half, "lin": flat})["vgg"]["features.0.weight"].dtype == torch.float32


def test_loader_refuses(weights):
    from ccvs_amd.tools.pytorch_metrics.lpips import load_lpips_weights
    missing = {k: v for k, v in weights["vgg"].items() if k != "features.17.bias"}
    with pytest.raises(ValueError, match=r"features\.17\.bias"):
        load_lpips_weights({"vgg": missing, "lin": weights["lin"]})
    wrong = dict(weights["vgg"])
    wrong["features.5.weight"] = torch.zeros(128, 64, 1, 1)
    with pytest.raises(ValueError, match=r"features\.5\.weight"):
        load_lpips_weights({"vgg": wrong, "lin": weights["lin"]})
    with pytest.raises(ValueError, match="4 heads"):
        load_lpips_weights({"vgg": weights["vgg"], "lin": weights["lin"][:4]})
    heads = {f"lin{i}.model.1.weight": t for i, t in enumerate(weights["lin"])}
    heads["lin2.model.1.weight"] = torch.zeros(1, 255, 1, 1)
    with pytest.raises(ValueError, match=r"lin2\.model\.1\.weight"):
        load_lpips_weights({"vgg": weights["vgg"], "lin": heads})
    with pytest.raises(ValueError, match='"vgg" and "lin"'):
        load_lpips_weights({"vgg": weights["vgg"]})
    with pytest.raises(ValueError, match="not a tensor"):
        load_lpips_weights({"vgg": dict(weights["vgg"], **{"features.0.bias": [0.0] * 64}), "lin": weights["lin"]})


def test_converter_round_trip(weights, tmp_path):
    from ccvs_amd.tools.pytorch_metrics import lpips as L
    vgg = dict(weights["vgg"])
    vgg["classifier.6.bias"] = torch.zeros(1000)
    torch.save(vgg, tmp_path / "vgg16.pth")
    torch.save({f"lin{i}.model.1.weight": t for i, t in enumerate(weights["lin"])}, tmp_path / "heads.pt")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = subprocess.run([sys.executable, "-m", "ccvs_amd.tools.pytorch_metrics.lpips", "--vgg", str(tmp_path / "vgg16.pth"), "--lin",
                          str(tmp_path / "heads.pt"), "--out", str(tmp_path / "lpips_vgg16.pt")], env=env, cwd=ROOT, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    got = L.load_lpips_weights(tmp_path / "lpips_vgg16.pt")
    assert sorted(got["vgg"]) == sorted(weights["vgg"]) and all(torch.equal(got["vgg"][k], weights["vgg"][k]) for k in weights["vgg"])
    assert all(torch.equal(a, b) for a, b in zip(got["lin"], weights["lin"]))
    args = L.parse_args(["--vgg", "a", "--lin", "b", "--out", "c"])
    assert (args.vgg, args.lin, args.out) == ("a", "b", "c")
    torch.save(list(weights["lin"]), tmp_path / "list.pt")      # the heads as a plain list
    assert all(torch.equal(a, b) for a, b in zip(L.convert(tmp_path / "vgg16.pth", tmp_path / "list.pt", tmp_path / "o.pt")["lin"], weights["lin"]))


# ------------------------------------------------------------------ 3: the C ABI
def test_lpips_symbols_declared_and_exported(tmp_path):
    from ccvs_amd import lib
    header = open(os.path.join(ROOT, "include", "ccvs_hip_lpips.h")).read()
    assert re.search(r'^#include "ccvs_hip_lpips.h"', open(os.path.join(ROOT, "include", "ccvs_hip.h")).read(), re.M)
    declared = sorted(set(re.findall(r"^(?:int64_t|int) (ccvs_[a-zA-Z0-9_]+)\s*\(", header, re.M)))
    assert declared == sorted(lib.LPIPS_EXPORTS) == ["ccvs_lpips_layer", "ccvs_lpips_layer_workspace_bytes", "ccvs_lpips_prep", "ccvs_relu_", "ccvs_relu_maxpool2"]
    others = (set(lib.EXPORTS) | set(lib.EVAL_EXPORTS) | set(lib.INPUT_EXPORTS) | set(lib.GEMM_EXPORTS) | set(lib.OUTPUT_EXPORTS) | set(lib.DECODE_EXPORTS)
              | set(lib.VIDEO_EXPORTS) | set(lib.OUTPUT_SAMPLED_EXPORTS))
    assert not set(lib.LPIPS_EXPORTS) & others and len(lib.EXPORTS) == 51
    handle = ctypes.CDLL(lib.LIB_PATH)
    for sym in lib.LPIPS_EXPORTS:
        assert hasattr(handle, sym), sym
    c = tmp_path / "p.c"
    c.write_text('#include "ccvs_hip.h"\nvoid* p[] = {' + ", ".join("(void*)" + s for s in lib.LPIPS_EXPORTS) + "};\n")
    subprocess.run(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(c), "-o", str(tmp_path / "p.o")], check=True)
    L = lib.load()
    assert L.ccvs_abi_version() == 6
    ws = L.ccvs_lpips_layer_workspace_bytes
    assert ws(32, 256 * 256) == 8 * 32 * 1024 and ws(1, 1) == 8 and ws(3, 65) == 8 * 3 * 2
    assert ws(0, 4) == 0 and ws(65536, 4) == 0 and ws(1, 0) == 0
    # refused before any GPU call
    one = ctypes.c_void_p(16)
    f3 = (ctypes.c_float * 3)(1, 1, 1)
    for call, word in ((lambda: L.ccvs_lpips_prep(one, one, 4, 16, f3, f3, None), "multiple of 3"), (lambda: L.ccvs_lpips_prep(one, one, 3, 0, f3, f3, None), "HW"),
                       (lambda: L.ccvs_lpips_prep(None, one, 3, 16, f3, f3, None), "null"), (lambda: L.ccvs_relu_(one, 0, None), "no elements"),
                       (lambda: L.ccvs_relu_(None, 4, None), "null"), (lambda: L.ccvs_relu_maxpool2(one, one, 1, 1, 8, None), "2 x 2"),
                       (lambda: L.ccvs_relu_maxpool2(one, None, 1, 8, 8, None), "null"), (lambda: L.ccvs_lpips_layer(one, one, one, one, 65536, 8, 4, 1, 0, None), "65535"),
                       (lambda: L.ccvs_lpips_layer(one, one, one, one, 1, 0, 4, 1, 0, None), "C > 0"), (lambda: L.ccvs_lpips_layer(one, one, one, None, 1, 8, 4, 1, 0, None), "null")):
        assert call() != 0
        assert word in L.ccvs_last_error().decode(), (word, L.ccvs_last_error().decode())


def test_ops_refuse_before_the_gpu():
    from ccvs_amd import lib, ops
    for call in (lambda: ops.lpips_prep(torch.zeros(1, 3, 4, 4)), lambda: ops.relu_(torch.zeros(4)), lambda: ops.relu_maxpool2(torch.zeros(1, 4, 4)),
                 lambda: ops.lpips_layer(torch.zeros(2, 4, 4), torch.zeros(4))):
        with pytest.raises(lib.CcvsError):
            call()


# ------------------------------------------------------------------ 4: the command
def test_command_line_and_the_state_without_weights(M, capsys, monkeypatch):
    monkeypatch.delenv("CCVS_LPIPS_WEIGHTS", raising=False)
    assert M.parse_args(["--exp_tag", "t"]).lpips_weights is None
    assert M.parse_args(["--exp_tag", "t", "--lpips_weights", "w.pt", "--print_256"]).lpips_weights == "w.pt"
    with pytest.raises(NotImplementedError):
        M.get_lpips(None, None)
    M.print_scores([None], "LPIPS")
    assert capsys.readouterr().out.splitlines() == ["LPIPS scores: not available (needs pretrained weights)"]
    assert M._lpips_lists([]) is None and M._lpips_lists([0, 2]) is None
    # the aggregate without LPIPS lists returns None in its place and prints the line there was
    s, p = [torch.tensor(0.5, dtype=torch.float64)] * 32, [torch.tensor(20.0)] * 32
    assert M._aggregate(s, p, True, [], 16)[0] is None
    assert capsys.readouterr().out.startswith("(256) SSIM is 0.5 (+- ")
    lp, sm, pm = M._aggregate(s, p, True, [], 16, [torch.tensor(0.25)] * 32)
    assert lp.item() == 0.25 and sm.item() == 0.5 and pm.item() == 20.0
    assert capsys.readouterr().out.startswith("(256) LPIPS is: 0.25 (+- ")
    lp, _, _ = M._aggregate([s, s], [p, p], False, [0, 2], 16, [[torch.tensor(0.25)] * 2, [torch.tensor(0.75)] * 2])
    assert [v.item() for v in lp] == [0.25, 0.75]
