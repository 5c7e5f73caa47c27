"""Shared checks of the kernel-level GPU tests (a plain module, imported by name like f32_autograd).

Output buffers start out as a non-canonical NaN bit pattern (`sent`), so a test can tell both that
every element a kernel owns was written and that nothing else was touched; `okey` / `ulps` measure
distances in units in the last place, `table` packs a launch table the way the engines do;
`pack_bits`, `pool_ref` and `pool_bwd_ref` are the plain references of the ReLU bit masks and of
the 3x3 / stride-2 max-pool that several kernels fuse.

The matrix-core kernel tests (test_gpu_fused_kernels.py, test_gpu_gemm_kernels.py,
test_gpu_conv_f32_kernels.py) share their host-generated inputs (`gen`, `tern`, `ints`, `pick`,
`randn`, `bn`) and their two checks: `check_exact` (small integers: bit for bit against fp64,
`precond` asserting on the reference that fp32 accumulation is exact) and `check_real` (a
per-element error bound), `check_bits` / `untouched` for the ReLU bit outputs; `gather` is the
fp64 im2col of the implicit GEMMs and `guards_only` the check of a split-K workspace.
"""
import torch
import torch.nn.functional as F

dev = "cuda"
SENT16 = 0x7FA5          # bf16 sentinel: a NaN no kernel here produces
SENT32 = 0x7FA5A5A5      # fp32 sentinel
U = 2.0 ** -24           # fp32 unit round-off
GUARD = 16               # sentinel elements before and after every guarded output


def sent(n, dtype):
    if dtype == torch.bfloat16:
        return torch.full((n,), SENT16, dtype=torch.int16, device=dev).view(torch.bfloat16)
    return torch.full((n,), SENT32, dtype=torch.int32, device=dev).view(torch.float32)


def bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def is_sent(t):
    return bits(t) == (SENT16 if t.element_size() == 2 else SENT32)


def okey(t):
    """Bit pattern -> integer that orders like the value: differences are distances in ulps."""
    if t.element_size() == 2:
        b = t.view(torch.int16).to(torch.int32)
        return torch.where(b < 0, -(b & 0x7FFF), b)
    b = t.view(torch.int32).to(torch.int64)
    return torch.where(b < 0, -(b & 0x7FFFFFFF), b)


def ulps(got, want):
    return (okey(got.contiguous()) - okey(want.contiguous())).abs()


def rel64(got, ref):
    return ((got.double() - ref).norm() / (ref.norm() + 1e-300)).item()


def table(rows):
    return torch.frombuffer(bytearray(b"".join(rows)), dtype=torch.uint8).clone().to(dev)


class Out:
    """An output of n elements inside GUARD sentinels; `start` preloads it (accumulators, in-place)."""

    def __init__(self, n, dtype, start=None):
        self.buf = sent(n + 2 * GUARD, dtype)
        self.n = n
        self.t = self.buf[GUARD:GUARD + n]
        if start is not None:
            self.t.copy_(start.reshape(-1))

    def check(self, what, owned=None):
        assert bool(is_sent(self.buf[:GUARD]).all()) and bool(is_sent(self.buf[GUARD + self.n:]).all()), \
            f"{what}: guard overwritten"
        s = is_sent(self.t)
        if owned is None:
            assert not bool(s.any()), f"{what}: {int(s.sum())} owned elements not written"
        else:
            assert not bool(s[owned].any()), f"{what}: owned elements not written"
            assert bool(s[~owned].all()), f"{what}: wrote outside what it owns"


class ByteOut:
    """A uint8 output (bit masks, argmax taps) of n bytes, preset to 0xA5, inside 0xA5 guard bytes."""

    def __init__(self, n):
        self.buf = torch.full((n + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=dev)
        self.n = n
        self.t = self.buf[GUARD:GUARD + n]

    def check(self, what):
        assert bool((self.buf[:GUARD] == 0xA5).all()) and bool((self.buf[GUARD + self.n:] == 0xA5).all()), \
            f"{what}: bits guard overwritten"


def pack_bits(y):
    w = (y.float() > 0).reshape(-1, 8).to(torch.int32)
    return (w << torch.arange(8, device=dev, dtype=torch.int32)).sum(-1).to(torch.uint8)


# ------------------------------------------------------------------------------- inputs
# (from a host generator, so the references and the exact-case preconditions are the same on any device)
BF, F32 = torch.bfloat16, torch.float32
PRECOND = {}     # kernel -> (largest sum |a||b|, largest |ref| of an output that is summed afterwards)


def gen(seed):
    return torch.Generator().manual_seed(seed)


def tern(g, *shape, p=0.25):
    """{-1, 0, 1}, nonzero with probability p."""
    s = torch.randint(0, 2, shape, generator=g) * 2 - 1
    return (s * (torch.rand(shape, generator=g) < p)).to(BF).to(dev)


def ints(g, lo, hi, *shape, dtype=BF):
    return torch.randint(lo, hi + 1, shape, generator=g).to(dtype).to(dev)


def pick(g, vals, n):
    return torch.tensor(vals, dtype=F32)[torch.randint(0, len(vals), (n,), generator=g)].to(dev)


def randn(g, *shape, scale=1.0, dtype=BF):
    return (torch.randn(shape, generator=g) * scale).to(dtype).to(dev)


def bn(g, n, exact):
    """Folded-BN scale / shift of n channels."""
    if exact:
        return pick(g, (0.5, 1.0, 2.0), n), ints(g, -3, 3, n, dtype=F32)
    return (torch.rand(n, generator=g) + 0.5).to(dev), randn(g, n, scale=0.1, dtype=F32)


# ------------------------------------------------------------------------------- checks
def precond(kernel, mag, summed=None):
    """Exact-case preconditions, on the reference alone: every sum of |a||b| below 2^24, and the
    outputs that are summed afterwards integers of magnitude <= 256."""
    m = float(mag.max())
    assert m < 2 ** 24, f"{kernel}: test bug, sum |a||b| = {m}"
    r = 0.0
    if summed is not None:
        r = float(summed.abs().max())
        assert r <= 256 and bool((summed == summed.round()).all()), f"{kernel}: test bug, |ref| = {r}"
    old = PRECOND.get(kernel, (0.0, 0.0))
    PRECOND[kernel] = (max(old[0], m), max(old[1], r))


def check_exact(got, ref64, what):
    """bf16: bit-identical to the rounded fp64 reference (which is an exact fp32 value, so its
    conversion rounds once; the sign of a zero aside).  fp32 and folded (fp64) sums: equal."""
    got, ref64 = got.reshape(-1), ref64.reshape(-1)
    if got.dtype == BF:
        bad = ulps(got, ref64.to(BF)) != 0
    else:
        bad = got.double() != ref64
    if bool(bad.any()):
        i = int(bad.nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ, the first at flat index {i}: "
                             f"{got[i].item()} for {ref64[i].item()} (norm-relative {rel64(got, ref64):.2e})")


def check_real(got, ref64, mag, K, what, rounded=True):
    """|got - ref| <= 2^-8 |ref| + (K + 4) U mag per element (`rounded`: a bf16 output)."""
    got, ref64, mag = got.double().reshape(-1), ref64.reshape(-1), mag.reshape(-1)
    bound = (K + 4) * U * mag + (2.0 ** -8 * ref64.abs() if rounded else 0.0)
    err = (got - ref64).abs()
    over = ~(err <= bound)
    worst = float((err / bound.clamp_min(1e-300)).nan_to_num(posinf=float("inf")).max())
    print(f"{what}: worst err / bound {worst:.3f}")
    if bool(over.any()):
        i = int(torch.where(over, err - bound, -1.0).nan_to_num(nan=float("inf")).argmax())
        raise AssertionError(f"{what}: {int(over.sum())} of {over.numel()} elements over the bound, the worst at flat "
                             f"index {i}: {got[i].item()} for {ref64[i].item()}, |err| {err[i].item():.3e} > "
                             f"{bound[i].item():.3e}")


def check(kind, got, ref64, mag, K, what, rounded=True):
    if kind == "exact":
        check_exact(got, ref64, what)
    else:
        check_real(got, ref64, mag, K, what, rounded)


def check_bits(bt, out, what):
    bt.check(what)
    assert torch.equal(bt.t, pack_bits(out.t)), f"{what}: bits != packed (stored output > 0)"


def untouched(bt, what):
    bt.check(what)
    assert bool((bt.t == 0xA5).all()), f"{what}: bits written without a bits buffer"


def nothing(n):
    return torch.zeros(n, dtype=torch.bool, device=dev)


def guards_only(o, what):
    """A workspace: whatever of it was written, the guards around it were not."""
    o.check(what, ~is_sent(o.t))


def gather(a, H, W, R, S, stride, pad, Ho, Wo):
    """The gathered A matrix by a scan over the taps, fp64: [N, H, W, C] -> [N Ho Wo, R S C] with
    k = (r S + s) C + c, zero outside the image."""
    n, C = a.shape[0], a.shape[-1]
    eh, ew = max(0, (Ho - 1) * stride + R - pad - H), max(0, (Wo - 1) * stride + S - pad - W)
    xp = F.pad(a.double().view(n, H, W, C), (0, 0, pad, ew, pad, eh))
    taps = [xp[:, r:r + (Ho - 1) * stride + 1:stride, s:s + (Wo - 1) * stride + 1:stride]
            for r in range(R) for s in range(S)]
    return torch.stack(taps, 3).reshape(n * Ho * Wo, R * S * C)


def pool_ref(x):
    """ZeroPadding2D(1) + 3x3 / stride 2 by a scan over the nine taps with strict '>': the first
    maximum in scan order wins.  x [B, H, W, C] (any float type; compared in fp64)."""
    B, H, W, C = x.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    xp = torch.zeros(B, H + 2, W + 2, C, dtype=torch.float64, device=dev)
    xp[:, 1:H + 1, 1:W + 1] = x.double()
    best = torch.full((B, Ho, Wo, C), float("-inf"), dtype=torch.float64, device=dev)
    tap = torch.zeros(B, Ho, Wo, C, dtype=torch.uint8, device=dev)
    for r in range(3):
        for s in range(3):
            v = xp[:, r:r + 2 * Ho - 1:2, s:s + 2 * Wo - 1:2]
            up = v > best
            best = torch.where(up, v, best)
            tap = torch.where(up, torch.full_like(tap, r * 3 + s), tap)
    return best, tap


def pool_bwd_ref(gy, tap, xmask, H, W):
    """Route each output gradient to its tap; taps in the padding are dropped; ReLU mask of x."""
    B, Ho, Wo, C = gy.shape
    gp = torch.zeros(B, H + 2, W + 2, C, dtype=torch.float64, device=dev)
    for r in range(3):
        for s in range(3):
            gp[:, r:r + 2 * Ho - 1:2, s:s + 2 * Wo - 1:2] += torch.where(tap == r * 3 + s, gy.double(), 0.0)
    gx = gp[:, 1:H + 1, 1:W + 1]
    return gx if xmask is None else gx * (xmask.double() > 0)
