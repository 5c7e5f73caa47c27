"""The per-step parameter pipeline, kernel by kernel, against fp64 PyTorch.

  prep / prep_fuse / prep_f32 : fp32 master -> forward weights, transposed + flipped + BN-scaled
                                dgrad weights, fused projection weights, folded scale / shift
  wgrad_finalize -> bn_grad   : column sums + raw weight gradients -> bias / gamma / beta gradients
  cast_bf16 / cast_f32 / scale_ / adam / sgd : the gradient wire and the update

Tables are packed with the engine's own struct formats.  Every output buffer starts out as a
non-canonical NaN bit pattern, so each test checks both that every element a kernel owns was
written and that nothing else was touched.  bf16 results are compared in integer ulps against the
fp64 value rounded once.
"""
import math
import struct
from types import SimpleNamespace as NS

import pytest
import torch
import torch.nn.functional as F

from pddl.models.engine import _BNG_FMT, _FIN_FMT, _FUSE_FMT, _PREP_FMT, IGEMM_DGRAD, STEM_K
from pddl.models.resnet50 import BN_EPS

from kernel_checks import SENT16, SENT32, U, bits, dev, is_sent, rel64, sent, table, ulps

pytestmark = pytest.mark.gpu

EPS = float(torch.tensor(BN_EPS, dtype=torch.float32))   # the value the kernels receive
ULP1_SHARE = 1e-3        # cap on the share of bf16 elements off by exactly one ulp


def N():
    from pddl.ops.native import require_native
    return require_native()


class Alloc:
    """Offsets in a flat buffer: multiples of 8, a gap (>= 8 sentinel elements) between regions."""

    def __init__(self):
        self.off = 8

    def take(self, n):
        o = self.off
        self.off = (o + n + 8 + 7) // 8 * 8
        return o


def pack_prep(r):
    return struct.pack(_PREP_FMT, r.w, r.cout, r.R, r.R, r.cin, r.kpad, r.wf, r.wd, r.ld, r.bias, r.gamma, r.beta,
                       r.mean, r.var, r.ch, r.mode)


def fold_ref(P, cout, bias, gamma, beta, mean, var):
    """fp64 folded frozen-BN affine (a, b) of one layer and the magnitude its fp32 rounding
    error scales with; absent offsets (-1) mean gamma 1, var 1 - eps, the others 0."""
    def vec(off, default):
        return P[off:off + cout] if off >= 0 else torch.full((cout,), default, dtype=torch.float64, device=P.device)
    g, v = vec(gamma, 1.0), vec(var, 1.0 - EPS)
    a = g / torch.sqrt(v + EPS) if (gamma >= 0 or var >= 0) else torch.ones_like(g)
    d = vec(bias, 0.0) - vec(mean, 0.0)
    be = vec(beta, 0.0)
    return a, d * a + be, d.abs() * a.abs() + be.abs()


def dgrad_ref(W, a):
    """W'[c][R-1-r][S-1-s][co] = a[co] * W[co][r][s][c] in fp64 (W is [cout][R][S][cin])."""
    return (W.double() * a.view(-1, 1, 1, 1)).flip(1).flip(2).permute(3, 1, 2, 0).contiguous()


class UlpCount:
    """The bf16 rule: nothing off by more than one ulp, at most ULP1_SHARE off by exactly one."""

    def __init__(self):
        self.worst, self.n1, self.n = 0, 0, 0

    def add(self, got, ref64):
        d = ulps(got, ref64.to(torch.bfloat16))
        self.worst = max(self.worst, int(d.max()))
        self.n1 += int((d == 1).sum())
        self.n += d.numel()

    def check(self, what):
        print(f"{what}: {self.n} bf16 elements, worst {self.worst} ulp, {self.n1} off by one "
              f"(share {self.n1 / max(self.n, 1):.2e})")
        assert self.worst <= 1, f"{what}: an element is {self.worst} bf16 ulps off"
        assert self.n1 <= ULP1_SHARE * self.n, f"{what}: {self.n1} of {self.n} elements one ulp off"


def check_affine(P, r, scale, shift, ch_owned):
    a, b, mag = fold_ref(P, r.cout, r.bias, r.gamma, r.beta, r.mean, r.var)
    sl = slice(r.ch, r.ch + r.cout)
    assert not is_sent(scale[sl]).any() and not is_sent(shift[sl]).any(), f"{r.name}: affine not written"
    du = ulps(scale[sl], a.float())
    assert int(du.max()) <= 4, f"{r.name}: scale {int(du.max())} fp32 ulps from gamma / sqrt(var + eps)"
    err = (shift[sl].double() - b).abs()
    assert bool((err <= 4 * U * mag).all()), f"{r.name}: shift error {(err / (U * mag + 1e-300)).max().item():.2f} u"
    ch_owned[sl] = True


def check_prep(params, rows, wbf, scale, shift, parts=3, owned=None, ch_owned=None, what="prep"):
    """Everything `prep` / `prep_f32` owns for these rows and parts against the fp64 reference,
    and the sentinel everywhere else (unless the caller goes on marking `owned`)."""
    f32 = wbf.dtype == torch.float32
    final = owned is None
    if final:
        owned = torch.zeros(wbf.numel(), dtype=torch.bool, device=dev)
        ch_owned = torch.zeros(scale.numel(), dtype=torch.bool, device=dev)
    P = params.double()
    cnt = UlpCount()
    for r in rows:
        n = r.cout * r.R * r.R * r.cin
        W = params[r.w:r.w + n].view(r.cout, r.R, r.R, r.cin)
        if parts & 1:
            if r.mode == 1:   # stem: 7x7x3 taps scattered into [cout][4x4 windows][2x2 phases][4 ch], rest untouched
                want = sent(r.cout * STEM_K, wbf.dtype).view(r.cout, 4, 4, 2, 2, 4)
                for kr in range(r.R):
                    for ks in range(r.R):
                        want[:, kr // 2, ks // 2, kr % 2, ks % 2, :r.cin] = W[:, kr, ks, :].to(wbf.dtype)
                got = wbf[r.wf:r.wf + r.cout * STEM_K]
                assert torch.equal(bits(got), bits(want.view(-1))), f"{r.name}: stem scatter"
                assert int(is_sent(got).sum()) == r.cout * (STEM_K - r.R * r.R * r.cin)
                owned[r.wf:r.wf + r.cout * STEM_K] = True
            elif not f32:
                assert r.kpad == r.R * r.R * r.cin and r.w % 4 == 0 and r.wf % 4 == 0 and n % 4 == 0
                got = wbf[r.wf:r.wf + n]
                want = W.reshape(-1).cpu().to(torch.bfloat16).to(dev)   # (the host's round to nearest even)
                assert torch.equal(bits(got), bits(want)), f"{r.name}: forward weights"
                owned[r.wf:r.wf + n] = True
            check_affine(P, r, scale, shift, ch_owned)
        if parts & 2 and r.wd >= 0 and r.mode == 0:
            a = fold_ref(P, r.cout, r.bias, r.gamma, r.beta, r.mean, r.var)[0]
            shape, stride = (r.cin, r.R, r.R, r.cout), (r.R * r.R * r.ld, r.R * r.ld, r.ld, 1)
            got = wbf.as_strided(shape, stride, r.wd)
            assert not is_sent(got.contiguous()).any(), f"{r.name}: dgrad weights not all written"
            ref = dgrad_ref(W, a)
            if f32:
                du = ulps(got, ref.float())
                assert int(du.max()) <= 4, f"{r.name}: fp32 dgrad weight {int(du.max())} ulps off"
            else:
                one = UlpCount()
                one.add(got, ref)
                assert one.worst <= 1, f"{r.name}: a dgrad weight is {one.worst} bf16 ulps off"
                cnt.worst, cnt.n1, cnt.n = max(cnt.worst, one.worst), cnt.n1 + one.n1, cnt.n + one.n
            owned.as_strided(shape, stride, r.wd).fill_(True)
    if cnt.n:
        cnt.check(what + " dgrad weights")
    if final:
        check_untouched(wbf, owned, scale, shift, ch_owned, what)
    return owned, ch_owned


def check_untouched(wbf, owned, scale, shift, ch_owned, what):
    assert bool(is_sent(wbf)[~owned].all()), f"{what}: wrote outside its weight regions"
    assert bool(is_sent(scale)[~ch_owned].all()) and bool(is_sent(shift)[~ch_owned].all()), \
        f"{what}: wrote scale / shift outside the layers' channels"


# -------------------------------------------------------------------- 1. prep, synthetic
def _fill_bn(host, r, g):
    for off, kind in ((r.bias, "n"), (r.gamma, "u"), (r.beta, "n"), (r.mean, "n"), (r.var, "u")):
        if off >= 0:
            host[off:off + r.cout] = (0.5 + torch.rand(r.cout, generator=g)) if kind == "u" else \
                0.1 * torch.randn(r.cout, generator=g)


def _synth_rows():
    """One table: whole tile, partial tiles + pad columns, a projection pair sharing dgrad rows,
    a 3x3 layer of 648 tiles (a second round of the 576-workgroup grid), a dense-like layer,
    gamma-only, bare, no-dgrad, and the stem."""
    pa, wa, ca = Alloc(), Alloc(), Alloc()

    def row(name, cout, R, cin, bn, wd=None, ld=0, mode=0):
        r = NS(name=name, cout=cout, R=R, cin=cin, mode=mode, ld=ld)
        r.kpad = STEM_K if mode else R * R * cin
        r.w = pa.take(cout * R * R * cin)
        r.wf = wa.take(cout * r.kpad)
        r.bias, r.gamma, r.beta, r.mean, r.var = (pa.take(cout) if k in bn else -1 for k in "bgemv")
        r.ch = ca.take(cout)
        r.wd = wa.take(cin * R * R * ld) if wd == "own" else (-1 if wd is None else wd)
        return r

    rows = [row("whole_tile", 64, 1, 64, "bgemv", "own", 64),
            row("partial_tiles", 104, 1, 72, "bgemv", "own", 128)]
    c1 = row("proj_conv1", 40, 1, 80, "bgemv", "own", 40 + 72)
    rows += [c1, row("proj_conv0", 72, 1, 80, "bgemv", c1.wd + 40, 40 + 72),
             row("second_round_3x3", 520, 3, 460, "bgemv", "own", 520),
             row("dense_like", 1000, 1, 96, "b", "own", 1024),
             row("gamma_only", 48, 1, 32, "g", "own", 48),
             row("bare", 24, 1, 16, "", "own", 24),
             row("no_dgrad", 32, 1, 64, "bgemv"),
             row("stem", 64, 7, 3, "bgemv", mode=1)]
    assert 9 * ((520 + 63) // 64) * ((460 + 63) // 64) == 648   # > the kernel's 576 workgroups per layer
    return rows, pa.off, wa.off, ca.off


@pytest.fixture(scope="module")
def synth():
    rows, npar, nw, nch = _synth_rows()
    g = torch.Generator().manual_seed(21)
    host = torch.full((npar,), float("nan"))   # the gaps between tensors are never read
    for r in rows:
        n = r.cout * r.R * r.R * r.cin
        host[r.w:r.w + n] = 0.05 * torch.randn(n, generator=g)
        _fill_bn(host, r, g)
    # +-0, ties to even (down and up), bf16 denormals, round-ups into the next binade
    special = [0.0, -0.0, 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), 2.0 ** -130, 3 * 2.0 ** -135,
               1.9999999, -0.99999994]
    host[rows[0].w:rows[0].w + len(special)] = torch.tensor(special)
    s = NS(rows=rows, params=host.to(dev), nw=nw, nch=nch, tab=table([pack_prep(r) for r in rows]),
           max_el=max(r.cout * r.kpad for r in rows))

    def run(parts, bufs=None, dtype=torch.bfloat16):
        w, sc, sh = bufs or (sent(nw, dtype), sent(nch, torch.float32), sent(nch, torch.float32))
        if dtype == torch.bfloat16:
            N().prep(s.params, s.tab, len(rows), s.max_el, w, sc, sh, BN_EPS, parts=parts)
        else:
            N().prep_f32(s.params, s.tab, len(rows), w, sc, sh, BN_EPS)
        torch.cuda.synchronize()
        return w, sc, sh
    s.run = run
    return s


def test_prep_synthetic_table(synth):
    """Forward weights bitwise, dgrad weights under the bf16 ulp rule, scale within 4 fp32 ulps,
    |shift - ref| <= 4 * 2^-24 * (|bias - mean| * |a| + |beta|), sentinels everywhere else: the pad
    columns of cout_pad, the stem's 109 unused slots per row, a projection pair's neighbour's
    columns, the gaps between regions and the channels no layer owns."""
    w, sc, sh = synth.run(3)
    check_prep(synth.params, synth.rows, w, sc, sh, 3)
    r = synth.rows[1]   # the 24 pad columns of the 104 -> 128 layer, explicitly
    assert bool(is_sent(w.as_strided((r.cin, r.ld - r.cout), (r.ld, 1), r.wd + r.cout)).all())


def test_prep_parts(synth):
    """parts=1 writes only forward weights + affine, parts=2 only the dgrad regions, and one
    after the other is bitwise parts=3."""
    both = synth.run(3)
    fwd = synth.run(1)
    check_prep(synth.params, synth.rows, *fwd, 1)
    dg = synth.run(2)
    check_prep(synth.params, synth.rows, *dg, 2)
    assert bool(is_sent(dg[1]).all()) and bool(is_sent(dg[2]).all())
    seq = synth.run(2, fwd)
    for a, b in zip(seq, both):
        assert torch.equal(bits(a), bits(b))


def test_prep_dgrad_later_rounds_repeat():
    """Layers of 2304 and 1152 tiles: every workgroup of the 576-wide grid transposes several
    tiles through the same LDS tile, and only the barrier that ends a round keeps a wave that
    is ahead from loading the next tile over one the others still read.  Without it the result is
    wrong only when the waves drift apart: measured on an MI355X on this table's layers, 20 - 35 %
    of launches had a few wrong elements (the synthetic table's 648-tile layer: 0 of 50).  So the
    first launch is checked in full and 47 more must repeat it bit for bit, which leaves a missing
    barrier about 0.7^48 = 4e-8 to pass."""
    torch.manual_seed(28)
    pa, wa, ca = Alloc(), Alloc(), Alloc()
    rows = []
    for i, (cout, R, cin) in enumerate([(1024, 3, 1024)] * 2 + [(2000, 3, 200)] * 2):
        r = NS(name=f"rounds{i}", cout=cout, R=R, cin=cin, kpad=R * R * cin, mode=0, ld=cout, bias=-1, beta=-1, mean=-1)
        r.w, r.gamma, r.var, r.ch = pa.take(cout * R * R * cin), pa.take(cout), pa.take(cout), ca.take(cout)
        r.wf = wa.take(0)   # (only the dgrad part runs here: no forward region)
        r.wd = wa.take(cin * R * R * cout)
        rows.append(r)
    params = torch.randn(pa.off, device=dev) * 0.05
    for r in rows:
        params[r.gamma:r.gamma + r.cout] = torch.rand(r.cout, device=dev) + 0.5
        params[r.var:r.var + r.cout] = torch.rand(r.cout, device=dev) + 0.5
    tab = table([pack_prep(r) for r in rows])
    sc, sh = sent(ca.off, torch.float32), sent(ca.off, torch.float32)

    def launch():
        w = sent(wa.off, torch.bfloat16)
        N().prep(params, tab, len(rows), 4096, w, sc, sh, BN_EPS, parts=2)
        torch.cuda.synchronize()
        return w
    first = launch()
    check_prep(params, rows, first, sc, sh, 2)
    for i in range(47):
        assert torch.equal(bits(launch()), bits(first)), f"launch {i + 2} differs from the first"


# ------------------------------------------------------------- 2. prep -> igemm (dgrad)
def test_prep_dgrad_weights_feed_igemm():
    """The layout prep writes is the layout the data-gradient GEMM reads: dx from the prepared
    weights of one 3x3 layer against fp64 conv2d_input of a * g (bound of test_igemm_dgrad)."""
    torch.manual_seed(22)
    n, h, cin, co, R = 2, 9, 64, 128, 3
    pa, wa = Alloc(), Alloc()
    r = NS(name="c", cout=co, R=R, cin=cin, kpad=R * R * cin, mode=0, ld=co, ch=0)
    r.w = pa.take(co * R * R * cin)
    r.bias, r.gamma, r.beta, r.mean, r.var = (pa.take(co) for _ in range(5))
    r.wf, r.wd = wa.take(co * r.kpad), wa.take(cin * R * R * co)
    params = torch.randn(pa.off, device=dev) * 0.05
    params[r.gamma:r.gamma + co] = torch.rand(co, device=dev) + 0.5
    params[r.var:r.var + co] = torch.rand(co, device=dev) + 0.5
    wbf, sc, sh = sent(wa.off, torch.bfloat16), sent(co, torch.float32), sent(co, torch.float32)
    N().prep(params, table([pack_prep(r)]), 1, co * r.kpad, wbf, sc, sh, BN_EPS, parts=3)
    g = (torch.randn(n, h, h, co, device=dev)).to(torch.bfloat16)
    add = torch.randn(n, h, h, cin, device=dev).to(torch.bfloat16)
    mask = torch.randn(n, h, h, cin, device=dev).to(torch.bfloat16)
    out = sent(n * h * h * cin, torch.bfloat16).view(n, h, h, cin)
    wt = wbf[r.wd:r.wd + cin * R * R * co].view(cin, R * R * co)
    N().igemm(g, None, h, h, R, R, 1, R - 1 - 1, h, h, wt, IGEMM_DGRAD, None, None, None, mask, add, out, 0, None, 0, 0,
              0, h, h, None, None)
    torch.cuda.synchronize()
    P = params.double()
    a = fold_ref(P, co, r.bias, r.gamma, r.beta, r.mean, r.var)[0]
    W = P[r.w:r.w + co * R * R * cin].view(co, R, R, cin)
    ref = torch.nn.grad.conv2d_input((n, cin, h, h), W.permute(0, 3, 1, 2), (g.double() * a).permute(0, 3, 1, 2),
                                     stride=1, padding=1)
    ref = (ref.permute(0, 2, 3, 1) + add.double()) * (mask.double() > 0)
    assert not is_sent(out).any()
    assert rel64(out, ref) < 1e-2


# ------------------------------------------------------------------ 3. prep, real table
def check_fuse(params, frows, wbf, scale, shift, owned, ch_owned, what):
    P = params.double()
    cnt = UlpCount()
    for f in frows:
        a3, b3, m3 = fold_ref(P, f.cout, f.bias3, f.gamma3, f.beta3, f.mean3, f.var3)
        a0, b0, m0 = fold_ref(P, f.cout, f.bias0, f.gamma0, f.beta0, f.mean0, f.var0)
        W3 = P[f.w3:f.w3 + f.cout * f.k3].view(f.cout, f.k3)
        W0 = P[f.w0:f.w0 + f.cout * f.k0].view(f.cout, f.k0)
        n = f.cout * (f.k3 + f.k0)
        got = wbf[f.wf:f.wf + n]
        assert not is_sent(got).any(), f"{f.name}: fused weights not all written"
        cnt.add(got, torch.cat([a3[:, None] * W3, a0[:, None] * W0], 1).reshape(-1))
        owned[f.wf:f.wf + n] = True
        sl = slice(f.ch, f.ch + f.cout)
        assert torch.equal(scale[sl], torch.ones(f.cout, device=dev)), f"{f.name}: fused scale is not exactly 1"
        # each branch's b within its own fp32 bound (see check_affine), plus the rounding of their sum
        err = (shift[sl].double() - (b3 + b0)).abs()
        assert bool((err <= 4 * U * (m3 + m0) + U * (b3 + b0).abs()).all()), f"{f.name}: fused shift"
        ch_owned[sl] = True
    cnt.check(what + " fused projection weights")


def test_prep_real_table():
    """after_update() on the ResNet-50 engine's own tables: all of wbf / scale / shift against a
    reference laid out from L.convs, wf, wd and wd_ld (same assertions as the synthetic table),
    the fused projection blocks included when the engine runs them."""
    from pddl.models.engine import HipEngine
    from pddl.models.resnet50 import ParamLayout
    L = ParamLayout()
    he = HipEngine(L, 1, crop=32, image_size=32)
    L.init_params(he.params, 3)
    g = torch.Generator(device="cpu").manual_seed(11)
    host = he.params.cpu()
    for e in L.entries.values():   # (as tests/test_gpu_engine.py _engines: the fold is not the identity)
        sl = host[e.offset:e.offset + e.size]
        if e.kind in ("gamma", "moving_variance"):
            sl.copy_(0.5 + torch.rand(e.size, generator=g))
        elif e.kind in ("beta", "bias", "moving_mean"):
            sl.copy_(0.1 * torch.randn(e.size, generator=g))
    he.params.copy_(host.to(dev))
    bits(he.wbf).fill_(SENT16)
    bits(he.scale).fill_(SENT32)
    bits(he.shift).fill_(SENT32)
    he.after_update()
    torch.cuda.synchronize()

    def bn(c):
        return (L.off(c.name, "bias"), L.off(c.bn, "gamma"), L.off(c.bn, "beta"), L.off(c.bn, "moving_mean"),
                L.off(c.bn, "moving_variance"))

    rows = []
    for c in L.convs:
        r = NS(name=c.name, cout=c.cout, R=c.k, cin=c.cin, mode=int(c is L.stem), w=L.off(c.name, "kernel"),
               wf=he.wf[c.name], wd=he.wd.get(c.name, -1), ld=he.wd_ld.get(c.name, 0), ch=he.ch[c.name])
        r.kpad = STEM_K if r.mode else c.k * c.k * c.cin
        r.bias, r.gamma, r.beta, r.mean, r.var = bn(c)
        rows.append(r)
    rows.append(NS(name="dense", cout=he.num_classes, R=1, cin=2048, kpad=2048, mode=0, w=L.off("dense", "kernel"),
                   wf=he.wf["dense"], wd=he.wd["dense"], ld=he.wd_ld["dense"], ch=he.ch["dense"],
                   bias=L.off("dense", "bias"), gamma=-1, beta=-1, mean=-1, var=-1))
    assert he.wd_ld["dense"] == 1024 and all(r.wd >= 0 for r in rows[1:])
    owned = torch.zeros(he.wbf.numel(), dtype=torch.bool, device=dev)
    ch_owned = torch.zeros(he.nch, dtype=torch.bool, device=dev)
    check_prep(he.params, rows, he.wbf, he.scale, he.shift, 3, owned, ch_owned, "engine")
    if he.fuse_proj:
        frows = []
        for b in L.blocks:
            if b.proj:
                c3, c0 = b.convs["3"], b.convs["0"]
                f = NS(name="fuse:" + b.name, cout=c3.cout, k3=c3.cin, k0=c0.cin, w3=L.off(c3.name, "kernel"),
                       w0=L.off(c0.name, "kernel"), ch=he.ch["fuse:" + b.name], wf=he.wf["fuse:" + b.name])
                f.bias3, f.gamma3, f.beta3, f.mean3, f.var3 = bn(c3)
                f.bias0, f.gamma0, f.beta0, f.mean0, f.var0 = bn(c0)
                frows.append(f)
        assert len(frows) == 4
        check_fuse(he.params, frows, he.wbf, he.scale, he.shift, owned, ch_owned, "engine")
    check_untouched(he.wbf, owned, he.scale, he.shift, ch_owned, "engine")


# ------------------------------------------------------------------------ 4. prep_fuse
def test_prep_fuse():
    """bf16(a3 * W3 | a0 * W0) under the ulp rule, scale exactly 1, shift = b3 + b0; a layer
    whose shortcut has no BN, and one of 270 400 elements (more than the 1024 x 256 threads)."""
    g = torch.Generator().manual_seed(23)
    pa, wa, ca = Alloc(), Alloc(), Alloc()
    frows = []
    for name, cout, k3, k0, bn0 in (("no_bn0", 72, 40, 24, False), ("grid_stride", 520, 320, 200, True)):
        f = NS(name=name, cout=cout, k3=k3, k0=k0, w3=pa.take(cout * k3), w0=pa.take(cout * k0))
        f.bias3, f.gamma3, f.beta3, f.mean3, f.var3 = (pa.take(cout) for _ in range(5))
        f.bias0 = pa.take(cout)
        f.gamma0, f.beta0, f.mean0, f.var0 = (pa.take(cout) if bn0 else -1 for _ in range(4))
        f.ch, f.wf = ca.take(cout), wa.take(cout * (k3 + k0))
        frows.append(f)
    assert 520 * 520 > 1024 * 256
    host = torch.full((pa.off,), float("nan"))
    for f in frows:
        for w, k in ((f.w3, f.k3), (f.w0, f.k0)):
            host[w:w + f.cout * k] = 0.05 * torch.randn(f.cout * k, generator=g)
        _fill_bn(host, NS(cout=f.cout, bias=f.bias3, gamma=f.gamma3, beta=f.beta3, mean=f.mean3, var=f.var3), g)
        _fill_bn(host, NS(cout=f.cout, bias=f.bias0, gamma=f.gamma0, beta=f.beta0, mean=f.mean0, var=f.var0), g)
    params = host.to(dev)
    tab = table([struct.pack(_FUSE_FMT, f.cout, f.k3, f.k0, f.w3, f.w0, f.bias3, f.gamma3, f.beta3, f.mean3, f.var3,
                             f.bias0, f.gamma0, f.beta0, f.mean0, f.var0, f.ch, f.wf) for f in frows])
    wbf, sc, sh = sent(wa.off, torch.bfloat16), sent(ca.off, torch.float32), sent(ca.off, torch.float32)
    N().prep_fuse(params, tab, len(frows), max(f.cout * (f.k3 + f.k0) for f in frows), wbf, sc, sh, BN_EPS)
    torch.cuda.synchronize()
    owned = torch.zeros(wa.off, dtype=torch.bool, device=dev)
    ch_owned = torch.zeros(ca.off, dtype=torch.bool, device=dev)
    check_fuse(params, frows, wbf, sc, sh, owned, ch_owned, "prep_fuse")
    check_untouched(wbf, owned, sc, sh, ch_owned, "prep_fuse")


# ------------------------------------------------------------------------- 5. prep_f32
def test_prep_f32(synth):
    """The fp32 engine's form on the same table: the stem's space-to-depth copy is the master
    bit for bit, dgrad weights within 4 fp32 ulps of fp64, scale / shift as in bf16, and the
    non-stem forward regions (that engine's convs read the master) untouched."""
    w, sc, sh = synth.run(3, dtype=torch.float32)
    owned, _ = check_prep(synth.params, synth.rows, w, sc, sh, 3)
    for r in synth.rows:
        if r.mode == 0:
            assert not owned[r.wf:r.wf + r.cout * r.kpad].any() and bool(is_sent(w[r.wf:r.wf + r.cout * r.kpad]).all())


# ------------------------------------------------------- 6. wgrad_finalize -> bn_grad
def test_bn_grad_table():
    """bias / gamma / beta gradients against fp64 (1e-6 per tensor): a full layer, the dense row
    (no BN, no dgamma), a layer reading another layer's column sums (a projection block's conv0
    reads conv3's), one without a folded scale, and 2100 channels (a second pass of the
    8 x 256-thread grid); nothing else in grads is written."""
    g = torch.Generator().manual_seed(24)
    pa, ca = Alloc(), Alloc()
    lay = []
    for name, cout, bn, has_ch in (("full", 96, True, True), ("dense", 1000, False, True),
                                   ("shared_colsum", 96, True, True), ("no_scale", 40, True, False),
                                   ("second_pass", 2100, True, True)):
        l = NS(name=name, cout=cout, bias=pa.take(cout))
        l.gamma, l.beta, l.mean, l.var = (pa.take(cout) if bn else -1 for _ in range(4))
        l.ch = ca.take(cout) if has_ch else -1
        l.cs = lay[0].cs if name == "shared_colsum" else ca.take(cout)
        l.dg = ca.take(cout) if bn else -1
        lay.append(l)
    assert lay[4].cout > 8 * 256
    host = torch.randn(pa.off, generator=g)
    for l in lay:
        if l.var >= 0:
            host[l.var:l.var + l.cout] = 0.5 + torch.rand(l.cout, generator=g)
    params = host.to(dev)
    colsum = torch.randn(ca.off, generator=g).to(dev)
    dgr = torch.randn(ca.off, generator=g).to(dev)
    scale = (0.5 + torch.rand(ca.off, generator=g)).to(dev)
    grads = sent(pa.off, torch.float32)
    tab = table([struct.pack(_BNG_FMT, l.cout, l.ch, l.bias, l.gamma, l.beta, l.mean, l.var, l.cs, l.dg) for l in lay])
    N().bn_grad(params, grads, tab, len(lay), colsum, dgr, scale, BN_EPS)
    torch.cuda.synchronize()
    P, owned = params.double(), torch.zeros(pa.off, dtype=torch.bool, device=dev)
    for l in lay:
        c = l.cout
        sg = colsum[l.cs:l.cs + c].double()
        a = scale[l.ch:l.ch + c].double() if l.ch >= 0 else torch.ones(c, dtype=torch.float64, device=dev)
        want = {l.bias: a * sg}
        if l.gamma >= 0:
            want[l.beta] = sg
            want[l.gamma] = (dgr[l.dg:l.dg + c].double() + (P[l.bias:l.bias + c] - P[l.mean:l.mean + c]) * sg) \
                / torch.sqrt(P[l.var:l.var + c] + EPS)
        for off, ref in want.items():
            assert not is_sent(grads[off:off + c]).any(), l.name
            assert rel64(grads[off:off + c], ref) < 1e-6, l.name
            owned[off:off + c] = True
    assert bool(is_sent(grads)[~owned].all())


def test_finalize_bn_grad_chain_matches_autograd():
    """wgrad_finalize then bn_grad on the column sums and raw weight gradient of a tiny conv +
    frozen BN, y = a * (conv(x, W) + bias - mean) + beta, against torch.autograd.grad of
    (y * g).sum() in fp64: dW, dbias, dgamma, dbeta within 1e-5 (wgrad_finalize's bound)."""
    torch.manual_seed(25)
    n, h, cin, co, R = 2, 6, 8, 12, 3
    k = R * R * cin
    f64 = dict(dtype=torch.float64, device=dev)
    # fp32 values, so the device's copy of the parameters is exact
    x = torch.randn(n, cin, h, h, device=dev).double()
    gup = torch.randn(n, co, h, h, device=dev).double()
    W = (0.2 * torch.randn(co, cin, R, R, device=dev)).double().requires_grad_()
    bias, beta, mean = ((0.3 * torch.randn(co, device=dev)).double() for _ in range(3))
    gamma, var = ((0.5 + torch.rand(co, device=dev)).double() for _ in range(2))
    bias.requires_grad_(), beta.requires_grad_(), gamma.requires_grad_()
    a = gamma / torch.sqrt(var + EPS)
    y = a.view(1, -1, 1, 1) * (F.conv2d(x, W, padding=1) + (bias - mean).view(1, -1, 1, 1)) + beta.view(1, -1, 1, 1)
    dW, dbias, dgamma, dbeta = torch.autograd.grad((y * gup).sum(), (W, bias, gamma, beta))
    # the device side: flat buffers [W (OHWI) | bias | gamma | beta | mean | var]
    o_w, o_b, o_g, o_be, o_m, o_v = 8, 8 + co * k, 8 + co * k + 16, 8 + co * k + 32, 8 + co * k + 48, 8 + co * k + 64
    ntot = o_v + 16
    params = torch.zeros(ntot, device=dev)
    params[o_w:o_w + co * k] = W.detach().permute(0, 2, 3, 1).reshape(-1).float()
    for o, t in ((o_b, bias), (o_g, gamma), (o_be, beta), (o_m, mean), (o_v, var)):
        params[o:o + co] = t.detach().float()
    grads = sent(ntot, torch.float32)
    dW_raw = torch.nn.grad.conv2d_weight(x, (co, cin, R, R), gup, padding=1)
    grads[o_w:o_w + co * k] = dW_raw.permute(0, 2, 3, 1).reshape(-1).float()
    ch, cs, dg = 4, 24, 40
    colsum = sent(64, torch.float32)
    colsum[cs:cs + co] = gup.sum((0, 2, 3)).float()
    scale = sent(64, torch.float32)
    scale[ch:ch + co] = a.detach().float()
    dgr = sent(64, torch.float32)
    N().wgrad_finalize(params, grads, table([struct.pack(_FIN_FMT, o_w, co, k, ch, dg)]), 1, scale, dgr, co)
    N().bn_grad(params, grads, table([struct.pack(_BNG_FMT, co, ch, o_b, o_g, o_be, o_m, o_v, cs, dg)]), 1, colsum, dgr,
                scale, BN_EPS)
    torch.cuda.synchronize()
    assert rel64(grads[o_w:o_w + co * k], dW.permute(0, 2, 3, 1).reshape(-1)) < 1e-5
    assert rel64(grads[o_b:o_b + co], dbias) < 1e-5
    assert rel64(grads[o_g:o_g + co], dgamma) < 1e-5
    assert rel64(grads[o_be:o_be + co], dbeta) < 1e-5
    owned = torch.zeros(ntot, dtype=torch.bool, device=dev)
    for o, m in ((o_w, co * k), (o_b, co), (o_g, co), (o_be, co)):
        owned[o:o + m] = True
    assert bool(is_sent(grads)[~owned].all())
    written = torch.zeros(64, dtype=torch.bool, device=dev)
    written[dg:dg + co] = True
    assert bool(is_sent(dgr)[~written].all()) and not is_sent(dgr)[written].any()


# -------------------------------------------------------- 7. casts, scale_, optimizers
CAST_N = 4096 * 256 + 1237      # past one pass of the 4096 x 256-thread grid
CAST_OFF, CAST_PAD = 3, 16      # an odd element offset inside a larger buffer
SPECIAL_F32 = [float("nan"), -float("nan"), float("inf"), -float("inf"), 0.0, -0.0, 1e-40, -1e-45, 2.0 ** -130,
               2.0 ** -134, 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), 1.9999999, 3.4028234663852886e38,
               -3.4028234663852886e38, float.fromhex("0x1.ffp127"), float.fromhex("0x1.fe8p127")]


@pytest.fixture(scope="module")
def cast_src():
    g = torch.Generator().manual_seed(26)
    x = torch.randn(CAST_N + CAST_PAD, generator=g) * torch.exp(4 * torch.randn(CAST_N + CAST_PAD, generator=g))
    sp = torch.tensor(SPECIAL_F32)
    x[CAST_OFF:CAST_OFF + len(sp)] = sp                          # both ends of the slice
    x[CAST_OFF + CAST_N - len(sp):CAST_OFF + CAST_N] = sp.flip(0)
    return x.to(dev)


def _same_bits_nan_aware(got, want):
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan)                    # a NaN stays a NaN
    assert torch.equal(bits(got)[~nan], bits(want)[~nan])


def test_cast_bf16(cast_src):
    """Bitwise `.to(torch.bfloat16)` (round to nearest even): ties, denormals, +-inf, the largest
    finite fp32 (rounds to inf), NaN stays NaN; the output's neighbours keep the sentinel."""
    sl = slice(CAST_OFF, CAST_OFF + CAST_N)
    y = sent(CAST_N + CAST_PAD, torch.bfloat16)
    N().cast_bf16(cast_src[sl], y[sl])
    torch.cuda.synchronize()
    want = cast_src[sl].cpu().to(torch.bfloat16).to(dev)         # (the host's round to nearest even)
    # the specials do what they are for: largest fp32 -> inf, tie above the largest bf16 -> inf, just below it -> finite
    assert torch.isinf(want[14]) and torch.isinf(want[-15]) and torch.isinf(want[16]) and torch.isfinite(want[17])
    assert want[10] == 1.0 and want[11] == 1 + 2.0 ** -6 and want[8] == 2.0 ** -130
    _same_bits_nan_aware(y[sl], want)
    assert bool(is_sent(y[:CAST_OFF]).all()) and bool(is_sent(y[CAST_OFF + CAST_N:]).all())


def test_cast_f32(cast_src):
    sl = slice(CAST_OFF, CAST_OFF + CAST_N)
    xb = cast_src.to(torch.bfloat16)
    y = sent(CAST_N + CAST_PAD, torch.float32)
    N().cast_f32(xb[sl], y[sl])
    torch.cuda.synchronize()
    assert torch.equal(bits(y[sl]), bits(xb[sl].float()))        # (exact, NaN payloads included)
    assert bool(is_sent(y[:CAST_OFF]).all()) and bool(is_sent(y[CAST_OFF + CAST_N:]).all())


def test_scale(cast_src):
    sl = slice(CAST_OFF, CAST_OFF + CAST_N)
    x = cast_src.clone()
    a = 0.3
    N().scale_(x[sl], a)
    torch.cuda.synchronize()
    _same_bits_nan_aware(x[sl], cast_src[sl] * torch.tensor(a, dtype=torch.float32, device=dev))
    assert torch.equal(bits(x[:CAST_OFF]), bits(cast_src[:CAST_OFF]))
    assert torch.equal(bits(x[CAST_OFF + CAST_N:]), bits(cast_src[CAST_OFF + CAST_N:]))


OPT_N = 4 * (4096 * 256) + 4 * 1237     # float4s: one full pass of the 4096 x 256-thread grid and a tail


@pytest.fixture(scope="module")
def opt_src():
    """Magnitudes of a training step (|p|, |g| ~ 0.5, momentum ~ 0.1, Adam v >= 1e-3).  On these
    very vectors an fp32 PyTorch re-implementation of every case below stays inside
    atol 1e-6 + rtol 1e-5 of the fp64 reference (checked on the CPU: worst error / allowance
    0.061 for sgd over the 16 flag combinations, 0.006 for adam), so the bound separates a wrong
    formula from fp32 rounding."""
    g = torch.Generator().manual_seed(27)
    r = lambda s: (s * torch.randn(OPT_N, generator=g)).to(dev)   # noqa: E731
    return NS(p=r(0.5), g=r(0.5), mom=r(0.1), m=r(0.05), v=(1e-3 + 0.1 * torch.rand(OPT_N, generator=g)).to(dev))


def _close(got, ref):
    return bool(((got.double() - ref).abs() <= 1e-6 + 1e-5 * ref.abs()).all())


@pytest.mark.parametrize("use_hs", [False, True])
@pytest.mark.parametrize("gscale", [1.0, 0.125])
@pytest.mark.parametrize("wd", [0.0, 1e-4])
@pytest.mark.parametrize("nesterov", [False, True])
def test_sgd_flags(opt_src, nesterov, wd, gscale, use_hs):
    """g' = g * gscale + wd * p;  v = mu v - lr g';  p += v  (Nesterov: p += mu v - lr g'), against
    fp64 at a size that runs the grid-stride loop and its tail; with `hs` the step size comes
    from hs[2] on the device and the host argument (deliberately wrong) is ignored."""
    lr, mu = 0.1, 0.9
    p, mom = opt_src.p.clone(), opt_src.mom.clone()
    hs = torch.tensor([3.0, 7.0, lr, 0.0], device=dev) if use_hs else None
    N().sgd(p, opt_src.g, mom, 123.0 if use_hs else lr, mu, wd, nesterov, gscale, hs)
    torch.cuda.synchronize()
    lr32, mu32, wd32, gs32 = (float(torch.tensor(v, dtype=torch.float32)) for v in (lr, mu, wd, gscale))
    p0, g0, v0 = opt_src.p.double(), opt_src.g.double(), opt_src.mom.double()
    gr = g0 * gs32 + wd32 * p0
    v1 = mu32 * v0 - lr32 * gr
    p1 = p0 + (mu32 * v1 - lr32 * gr if nesterov else v1)
    assert _close(mom, v1) and _close(p, p1)


def test_adam_gscale(opt_src):
    """Adam with gscale = 1/8 folded into the gradient, at the same size, against fp64."""
    lr_t, b1, b2, eps, gs = 1e-3 * math.sqrt(1 - 0.999 ** 3) / (1 - 0.9 ** 3), 0.9, 0.999, 1e-7, 0.125
    p, m, v = opt_src.p.clone(), opt_src.m.clone(), opt_src.v.clone()
    N().adam(p, opt_src.g, m, v, lr_t, b1, b2, eps, gs, None)
    torch.cuda.synchronize()
    lr32, b1_32, b2_32, eps32 = (float(torch.tensor(x, dtype=torch.float32)) for x in (lr_t, b1, b2, eps))
    gr = opt_src.g.double() * gs
    m1 = b1_32 * opt_src.m.double() + (1 - b1_32) * gr
    v1 = b2_32 * opt_src.v.double() + (1 - b2_32) * gr * gr
    p1 = opt_src.p.double() - lr32 * m1 / (v1.sqrt() + eps32)
    assert _close(m, m1) and _close(v, v1) and _close(p, p1)
