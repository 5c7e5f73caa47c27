"""conv2_block1's shortcut conv backward inside the fused conv3 backward (bwd1x1.hip dual form,
PDDL_ENGINE proj_bwd): the kernel against fp32 references and against today's three launches,
the launcher's argument checks, and the engine with the path on against the path off."""
import pytest
import torch

from pddl.utils.envopts import with_opt

pytestmark = pytest.mark.gpu

dev = "cuda"


def N():
    from pddl.ops.native import require_native
    return require_native()


def rel(a, b):
    a, b = a.float(), b.float()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


def rnd(*shape, scale=1.0):
    return (torch.randn(*shape, device=dev) * scale).to(torch.bfloat16)


def pack_bits(x):
    b = (x.float() > 0).to(torch.int32).view(*x.shape[:-1], x.shape[-1] // 8, 8)
    return (b << torch.arange(8, device=x.device, dtype=torch.int32)).sum(-1).to(torch.uint8)


GUARD, SENTINEL = 64, 123.0


def _guarded(M, C):
    """[M + GUARD][C] bf16: NaN in the M rows a launch must write, a sentinel in the guard rows."""
    t = torch.full((M + GUARD, C), float("nan"), device=dev, dtype=torch.bfloat16)
    t[M:] = SENTINEL
    return t


def _operands(M):
    torch.manual_seed(13)
    o = dict(g1=rnd(M, 64), w1d=rnd(256, 64, scale=0.05), add=rnd(M, 256), ox=rnd(M, 256), x=torch.relu(rnd(M, 64)),
             wd=rnd(64, 256, scale=0.05), x2=torch.relu(rnd(M, 64)), wd_all=rnd(64, 320, scale=0.05))
    o["gmask"], o["bits"] = pack_bits(o["ox"]), pack_bits(o["x"])
    o["wd2"] = o["wd_all"][:, 64:]          # a column slice: row stride 320
    o["dw0"] = torch.randn(256, 320, device=dev)
    return o


# 37: less than a tile; 200: a ragged 4th tile; 9,408: exact tiles, fewer than workgroups; 64,037:
# 1,001 tiles over one workgroup per CU (3-4 tiles each, unevenly, dW across tiles, ragged tail)
@pytest.mark.parametrize("M", [37, 200, 3 * 56 * 56, 64 * 1000 + 37])
def test_bwd1x1_dual_form(M):
    """out / dw / column sums as the pre form, out_s = g . wd2^T (no mask) and dw2 += g^T . x2 from
    the same g tile -- against fp32 torch, and against the pre-form launch writing g, the wgrad
    launch reading it and an fp32 product for the shortcut's data gradient.  With gx=None g is
    not written; with gx given the dual form still writes it.

    The 1e-3 bounds on dw, dw2 and the column sums of out are those of test_bwd1x1_fused, where g is
    an exact bf16 input; here g is computed, and the kernel (every form of it) holds the tile in
    LDS as bf16, so their fp32 reference rounds g to bf16 as well.  Against the unrounded g both
    this launch and the existing route sit at the rounding's own 1.6e-3 (M = 200: dw 1.59e-3, dw2
    1.59e-3, column sums 1.74e-3, and 5e-8 / 6e-8 / 0 between the two routes); those figures are
    printed as dw_f32 / dw2_f32 / cs_f32."""
    o = _operands(M)
    rows = N().bwd1x1_partial_rows(M, 256, 64, True)
    assert rows == min((M + 63) // 64, torch.cuda.get_device_properties(0).multi_processor_count) * 8
    out, out_s = _guarded(M, 64), _guarded(M, 64)
    cs = torch.full((rows * 64,), float("nan"), device=dev)
    csx = torch.full((rows * 256,), float("nan"), device=dev)
    dwa = o["dw0"].clone()
    dw, dw2 = dwa[:, :64], dwa[:, 64:128]   # two ranges of one pre-filled tensor with 320-float rows: ld_dw != 64
    pre = dict(g1=o["g1"], w1d=o["w1d"], gmask=o["gmask"])
    N().bwd1x1(o["add"], o["x"], o["wd"], o["bits"], out[:M], cs, dw, colsum_gx=csx, gx=None, x2=o["x2"],
               wd2=o["wd2"], out_s=out_s[:M], dw2=dw2, **pre)
    # the same launch with gx requested
    gx = _guarded(M, 256)
    out_g, outs_g = _guarded(M, 64), _guarded(M, 64)
    cs_g = torch.full((rows * 64,), float("nan"), device=dev)
    csx_g = torch.full((rows * 256,), float("nan"), device=dev)
    dwa_g = o["dw0"].clone()
    N().bwd1x1(o["add"], o["x"], o["wd"], o["bits"], out_g[:M], cs_g, dwa_g[:, :64], colsum_gx=csx_g, gx=gx[:M],
               x2=o["x2"], wd2=o["wd2"], out_s=outs_g[:M], dw2=dwa_g[:, 64:128], **pre)
    # the existing route: pre form writing gx_r, wgrad reading it, fp32 product
    rows_r = N().bwd1x1_partial_rows(M, 256, 64)
    gx_r = torch.empty(M, 256, device=dev, dtype=torch.bfloat16)
    out_r = torch.empty(M, 64, device=dev, dtype=torch.bfloat16)
    cs_r = torch.full((rows_r * 64,), float("nan"), device=dev)
    csx_r = torch.full((rows_r * 256,), float("nan"), device=dev)
    dw_r = torch.zeros(256, 64, device=dev)
    N().bwd1x1(o["add"], o["x"], o["wd"], o["bits"], out_r, cs_r, dw_r, gx=gx_r, colsum_gx=csx_r, **pre)
    dw2_r = torch.zeros(256, 64, device=dev)
    N().wgrad(o["x2"].view(1, 1, M, 64), 1, M, 1, 1, 1, 0, 1, M, gx_r.view(1, 1, M, 256), dw=dw2_r, K=64)
    torch.cuda.synchronize()
    outs_r = gx_r.float() @ o["wd2"].float().t()

    ref_gx = (o["g1"].float() @ o["w1d"].float().t() + o["add"].float()) * (o["ox"].float() > 0)
    ref = (ref_gx @ o["wd"].float().t()) * (o["x"] > 0)
    ref_s = ref_gx @ o["wd2"].float().t()
    ref_gb = ref_gx.bfloat16().float()       # g as the tile holds it
    ref_b = (ref_gb @ o["wd"].float().t()) * (o["x"] > 0)
    ref_dw, ref_dw2 = ref_gb.t() @ o["x"].float(), ref_gb.t() @ o["x2"].float()
    dw0a, dw0b = o["dw0"][:, :64], o["dw0"][:, 64:128]
    figs = dict(out=rel(out[:M], ref), out_s=rel(out_s[:M], ref_s), dw=rel(dw - dw0a, ref_dw),
                dw2=rel(dw2 - dw0b, ref_dw2), cs=rel(cs.view(rows, 64).sum(0), ref_b.sum(0)),
                dw_f32=rel(dw - dw0a, ref_gx.t() @ o["x"].float()), dw2_f32=rel(dw2 - dw0b, ref_gx.t() @ o["x2"].float()),
                cs_f32=rel(cs.view(rows, 64).sum(0), ref.sum(0)),
                csx=rel(csx.view(rows, 256).sum(0), ref_gx.sum(0)), gx=rel(gx[:M], ref_gx),
                out_vs=rel(out[:M], out_r), out_s_vs=rel(out_s[:M], outs_r), dw_vs=rel(dw - dw0a, dw_r),
                dw2_vs=rel(dw2 - dw0b, dw2_r), cs_vs=rel(cs.view(rows, 64).sum(0), cs_r.view(rows_r, 64).sum(0)),
                csx_vs=rel(csx.view(rows, 256).sum(0), csx_r.view(rows_r, 256).sum(0)))
    print(f"M={M}: " + ", ".join(f"{k} {v:.2e}" for k, v in figs.items()))
    assert figs["out"] < 1e-2 and figs["out_s"] < 1e-2
    assert figs["dw"] < 1e-3 and figs["dw2"] < 1e-3
    assert figs["cs"] < 1e-3 and figs["csx"] < 1e-3
    for k in ("out_vs", "out_s_vs", "dw_vs", "dw2_vs", "cs_vs", "csx_vs"):
        assert figs[k] < 5e-3, k
    # gx requested: written correctly, and everything else as without it
    assert figs["gx"] < 1e-2
    assert rel(out_g[:M], out[:M]) < 5e-3 and rel(outs_g[:M], out_s[:M]) < 5e-3 and rel(dwa_g, dwa) < 5e-3
    for t in (out, out_s, out_g, outs_g, gx):   # nothing past row M
        assert (t[M:] == SENTINEL).all()
    assert torch.equal(dwa[:, 128:], o["dw0"][:, 128:])   # ... nor beside the two dW ranges


def test_bwd1x1_dual_form_argument_checks():
    """Dual operands without the pre operands, CO = 512, the stride-2 form and ld_wd2 = 252 are
    refused before anything launches."""
    M = 128
    o = _operands(M)
    rows = N().bwd1x1_partial_rows(M, 256, 64, True)
    out, out_s = _guarded(M, 64), _guarded(M, 64)
    cs = torch.zeros(rows * 128, device=dev)
    csx = torch.zeros(rows * 256, device=dev)
    dw, dw2 = torch.zeros(256, 64, device=dev), torch.zeros(256, 64, device=dev)
    pre = dict(g1=o["g1"], w1d=o["w1d"], gmask=o["gmask"], colsum_gx=csx)
    dual = dict(x2=o["x2"], wd2=o["wd2"], out_s=out_s[:M], dw2=dw2)
    with pytest.raises(RuntimeError):   # no pre operands
        N().bwd1x1(o["add"], o["x"], o["wd"], o["bits"], out[:M], cs, dw, **dual)
    with pytest.raises(RuntimeError):   # CO = 512 (CI = 128)
        x128 = torch.relu(rnd(M, 128))
        N().bwd1x1(rnd(M, 512), x128, rnd(128, 512), pack_bits(x128), torch.empty_like(x128), cs,
                   torch.zeros(512, 128, device=dev), **pre, **dual)
    with pytest.raises(RuntimeError):   # stride-2 form
        N().bwd1x1(o["add"].view(2, 8, 8, 256), torch.relu(rnd(2, 16, 16, 64)), o["wd"],
                   torch.zeros(2, 16, 16, 8, dtype=torch.uint8, device=dev), torch.zeros(2, 16, 16, 64, device=dev,
                                                                                         dtype=torch.bfloat16),
                   cs, dw, torch.zeros(2, 8, 8, 64, device=dev, dtype=torch.bfloat16), **pre, **dual)
    with pytest.raises(RuntimeError):   # ld_wd2 = 252
        bad = dict(dual, wd2=torch.as_strided(rnd(64 * 252 + 8), (64, 256), (252, 1)))
        N().bwd1x1(o["add"], o["x"], o["wd"], o["bits"], out[:M], cs, dw, **pre, **bad)
    torch.cuda.synchronize()
    assert torch.isnan(out[:M].float()).all() and torch.isnan(out_s[:M].float()).all() and not dw2.any()


def _step(monkeypatch, key, value, B=8):
    from pddl.models.engine import HipEngine
    from pddl.models.resnet50 import ParamLayout
    monkeypatch.setenv("PDDL_ENGINE", with_opt("PDDL_ENGINE", key, value))
    he = HipEngine(ParamLayout(), B, crop=224, image_size=224)
    he.init(seed=7)
    img = torch.randint(0, 256, (B, 224, 224, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(1)).cuda()
    lab = torch.randint(0, 1000, (B,), generator=torch.Generator().manual_seed(2)).cuda()
    st = he.forward_backward(img, lab, 1.0 / B)
    torch.cuda.synchronize()
    return he, st[0].item() / B, he.grads.clone()


@pytest.mark.parametrize("two_stream", [None, "0"])
def test_proj_bwd_in_engine(monkeypatch, two_stream):
    """PDDL_ENGINE proj_bwd=1 (the default; forced on at this batch with proj_bwd_min_m) against 0: same loss, flat gradients to fp32 order plus
    the one bf16 rounding of the shortcut's data gradient (<= 2^-9 relative per element); B = 8
    takes the two-stream path by default, two_stream=0 the single stream.  And within the fp32
    reference's noise floor with the path on."""
    monkeypatch.setenv("PDDL_ENGINE", with_opt("PDDL_ENGINE", "proj_bwd_min_m", "1"))   # (default: from b64 up)
    if two_stream is not None:
        monkeypatch.setenv("PDDL_ENGINE", with_opt("PDDL_ENGINE", "two_stream", two_stream))
    res = []
    for on in ("1", "0"):
        he, loss, g = _step(monkeypatch, "proj_bwd", on)
        assert he.proj_bwd == (on == "1") and he._proj_bwd(0, he._s2_fed(), 8) == (on == "1")
        assert (he.side is not None) == (two_stream is None)
        res.append((loss, g))
    (l1, g1), (l0, g0) = res
    print(f"proj_bwd: loss rel {abs(l1 - l0) / abs(l0):.2e}, grad rel {((g1 - g0).norm() / g0.norm()).item():.3e}")
    assert abs(l1 - l0) < 1e-4 * abs(l0)
    assert ((g1 - g0).norm() / g0.norm()).item() < 3e-2
    if two_stream is None:
        from test_gpu_engine import test_engine_matches_bf16_point_reference_within_its_noise_floor as floor
        monkeypatch.setenv("PDDL_ENGINE", with_opt("PDDL_ENGINE", "proj_bwd", "1"))
        floor(224, 224)
