"""Shared checks of the kernel-level GPU tests (a plain module, imported by name like f32_autograd).

Output buffers start out as a non-canonical NaN bit pattern (`sent`), so a test can tell both that
every element a kernel owns was written and that nothing else was touched; `okey` / `ulps` measure
distances in units in the last place, `table` packs a launch table the way the engines do;
`pack_bits`, `pool_ref` and `pool_bwd_ref` are the plain references of the ReLU bit masks and of
the 3x3 / stride-2 max-pool that several kernels fuse.
"""
import torch

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
