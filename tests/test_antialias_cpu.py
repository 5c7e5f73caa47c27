"""--antialias on the CPU: the definition of csrc/kernels/kernels.h (`StemParams::antialias`) in fp64 (`ref64`, shared
with tests/test_gpu_antialias.py), TorchEngine's resample against it, and the flag's way to the config, banner and records."""
import json

import numpy as np
import torch

U = 2.0 ** -24


def axis64(o, n, N):
    """One axis of the definition: {box pixel: weight} of output index o, the weights summing to 1."""
    if n <= N:                                   # mode 3's two taps
        num = (2 * o + 1) * n - N
        t = num // (2 * N)
        f = (num - t * 2 * N) / (2 * N)
        lo, hi = min(max(t, 0), n - 1), min(max(t + 1, 0), n - 1)
        return {lo: 1.0} if lo == hi else {lo: 1 - f, hi: f}
    u = {i: 2 * n - abs((2 * i + 1) * N - (2 * o + 1) * n) for i in range(n)}
    D = sum(v for v in u.values() if v > 0)
    return {i: v / D for i, v in u.items() if v > 0}


def ref64(img, rows, flip, crop):
    """The definition in fp64 for in-range boxes: the raw 0..255 picture [B, crop, crop, 3] and the tap
    count T = T_y + T_x of every element [B, crop, crop, 1] (an unshrunk axis counts its two taps)."""
    out, taps = np.zeros((len(rows), crop, crop, 3)), np.zeros((len(rows), crop, crop, 1))
    for b, (y0, x0, h, w) in enumerate(rows):
        assert 0 <= y0 and 1 <= h and y0 + h <= img.shape[1] and 0 <= x0 and 1 <= w and x0 + w <= img.shape[2]
        Wy, Wx = np.zeros((crop, h)), np.zeros((crop, w))
        for o in range(crop):
            for i, v in axis64(o, h, crop).items():
                Wy[o, i] = v
            for i, v in axis64(crop - 1 - o if flip[b] else o, w, crop).items():
                Wx[o, i] = v
        out[b] = np.einsum("yi,ijc,xj->yxc", Wy, np.asarray(img[b, y0:y0 + h, x0:x0 + w], dtype=np.float64), Wx)
        ty, tx = (np.maximum((W > 0).sum(1), 2 if n <= crop else 1) for W, n in ((Wy, h), (Wx, w)))
        taps[b, :, :, 0] = ty[:, None] + tx[None, :]
    return out, taps


def test_torch_engine_resample_against_fp64():
    """Boxes shrunk on both axes, on one, on none, at a corner, one pixel wide; flips; the evaluation resize.  TorchEngine
    does not fuse: a product and a sum round per tap, 2T + 6 roundings of non-negative terms (crop 32: lerp weights exact)."""
    from pddl.models.reference import preprocess
    img = torch.randint(0, 256, (6, 75, 75, 3), generator=torch.Generator().manual_seed(5)).to(torch.uint8)
    rows = [(0, 0, 75, 75), (3, 7, 64, 64), (5, 5, 16, 70), (10, 3, 60, 1), (20, 20, 55, 55), (4, 6, 32, 16)]
    flip = torch.tensor([0, 1, 0, 0, 1, 1], dtype=torch.uint8)
    scale = float(np.float32(1) / np.float32(255))
    raw, T = ref64(img.numpy(), rows, flip.tolist(), 32)
    for src in (img, img.float()):
        got = preprocess(src, 32, True, flip, (0, 0), None, torch.tensor(rows, dtype=torch.int32), antialias=True).permute(0, 2, 3, 1).double().numpy()
        assert (np.abs(got - raw * scale) <= (2 * T + 6) * U * raw * scale).all()
    ev = preprocess(img[:2], 32, False, antialias=True).permute(0, 2, 3, 1).double().numpy()
    assert (np.abs(ev - raw[:1] * scale) <= (2 * T[:1] + 6) * U * raw[:1] * scale)[0].all()      # image 0's box is the whole source


def test_flag_config_banner_and_records(tmp_path, capsys):
    from pddl import cli
    from pddl.config import config_from_args
    assert config_from_args("single", ["--antialias"]).antialias is True and config_from_args("single", []).antialias is False
    common = ["--device", "cpu", "--batch-size", "4", "--crop", "32", "--image-size", "72", "--validation-steps", "1",
              "--no-save", "--verbose", "1", "--max-steps", "2", "--epochs", "1", "--rrc"]
    recs = {}
    for name, flags in (("aa", ["--antialias"]), ("plain", [])):
        jl = tmp_path / f"{name}.jsonl"
        assert cli.run("single", common + ["--metrics-jsonl", str(jl)] + flags) == 0
        assert f"antialias={bool(flags)}" in capsys.readouterr().out
        recs[name] = json.loads(jl.read_text().splitlines()[0])
    assert recs["aa"]["antialias"] is True and recs["plain"]["antialias"] is False and recs["aa"]["loss"] != recs["plain"]["loss"]
    assert {k: v for k, v in recs["aa"].items() if k != "antialias"}.keys() == {k for k in recs["plain"] if k != "antialias"}
