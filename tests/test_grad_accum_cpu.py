"""Gradient accumulation on CPU (--accum-steps): the accumulator's torch path, SingleStrategy on
the fp32 TorchEngine, two gloo Horovod ranks, and the configuration errors."""
import os

import pytest
import torch
import torch.multiprocessing as mp

SEED = 5
LR = 1e-2


def _cfg(preset, **kw):
    from pddl.config import make_config
    base = dict(device="cpu", data="synthetic", image_size=32, crop=32, flip=False, epochs=1, verbose=0, save=False,
                train_images=64, val_images=8, seed=SEED, lr=LR, optimizer="sgd", momentum=0.0)
    base.update(kw)
    return make_config(preset, **base)


def _per_tensor(L, a, b):
    """Largest per-tensor relative L2 difference of two flat trainable-prefix vectors (b: the reference)."""
    worst = (0.0, None)
    for e in L.entries.values():
        if not e.trainable:
            continue
        x, y = a[e.offset:e.offset + e.size].double(), b[e.offset:e.offset + e.size].double()
        r = ((x - y).norm() / (y.norm() + 1e-300)).item()
        if r > worst[0]:
            worst = (r, e.name + "/" + e.kind)
    return worst


def _engine(cap):
    from pddl.models.reference import TorchEngine
    from pddl.models.resnet50 import ParamLayout
    e = TorchEngine(ParamLayout(), cap, crop=32)
    e.init(seed=SEED)
    return e


@pytest.fixture(scope="module")
def ref8():
    """The first 8 training images of the synthetic source, their one-batch gradient (gscale 1/8)
    on unchanged code paths, and d_ref: the largest per-tensor relative L2 difference between
    that gradient and the gradient of the same 8 images in permuted order -- what fp32
    summation order alone does to this gradient."""
    from pddl.parallel.strategies import make_strategy
    from pddl.train.trainer import Trainer
    cfg = _cfg("single", batch_size=8)
    st = make_strategy(cfg)
    Trainer(cfg, st)
    img, lab = next(st.train_pipeline().iterate(st.device, epoch=0))
    assert img.shape[0] == 8
    e = _engine(8)
    e.forward_backward(img, lab, 1.0 / 8)
    g_one = e.grads.clone()
    perm = torch.tensor([5, 2, 7, 0, 3, 6, 1, 4])
    e.forward_backward(img[perm], lab[perm], 1.0 / 8)
    d_ref, where = _per_tensor(e.L, e.grads, g_one)
    assert d_ref > 0
    return dict(img=img, lab=lab, g_one=g_one, d_ref=d_ref, where=where, p0=e.params.clone(), L=e.L)


class _Eng:
    def __init__(self, n):
        self.grads = torch.zeros(n)


def test_accumulator_cpu_path_is_the_hand_written_sum():
    from pddl.train.accum import GradAccumulator
    torch.manual_seed(1)
    n, K = 1003, 4
    bks = [(0, 401), (401, 402), (402, 1000)]                      # [1000, 1003) lies outside every bucket
    eng = _Eng(n)
    acc = GradAccumulator(eng, K, bks)
    assert acc.acc.shape == eng.grads.shape and acc.acc.dtype == torch.float32
    seen = []
    for rnd in range(2):                                           # the counter wraps: two updates
        gs = [torch.randn(n) * 10.0 ** (m - 2) for m in range(K)]  # magnitudes differ: the order of additions shows
        want = ((gs[0] + gs[1]) + gs[2]) + gs[3]
        for m in range(K):
            eng.grads.copy_(gs[m])
            last = m == K - 1
            assert acc.last == last
            cb = acc.wrap(lambda i, m=m: seen.append((rnd, m, i)))
            for i in range(len(bks)):
                cb(i)
            assert acc.advance() == last
            if m == 0:
                assert torch.equal(acc.acc[:1000], gs[0][:1000])
            if not last:
                assert torch.equal(eng.grads, gs[m])
        assert torch.equal(eng.grads[:1000], want[:1000])
        assert torch.equal(eng.grads[1000:], gs[K - 1][1000:])
        assert want.ne((gs[3] + gs[2]) + (gs[1] + gs[0])).any()    # (another order does differ)
    assert seen == [(r, K - 1, i) for r in range(2) for i in range(len(bks))]
    # the whole-buffer form (no communication callback)
    eng2 = _Eng(n)
    acc2 = GradAccumulator(eng2, 2)
    a, b = torch.randn(n), torch.randn(n)
    eng2.grads.copy_(a)
    acc2.accumulate()
    assert not acc2.advance()
    eng2.grads.copy_(b)
    acc2.accumulate()
    assert acc2.advance()
    assert torch.equal(eng2.grads, a + b)
    with pytest.raises(ValueError):
        acc2.wrap(lambda i: None)                                  # no bucket layout
    for k in (1, 0, -2):
        with pytest.raises(ValueError):
            GradAccumulator(eng2, k)


def test_single_strategy_accumulates_four_micro_batches(ref8):
    """K = 4 micro-batches of 2 on the fp32 TorchEngine.  The gradient the optimizer reads is, bit
    for bit, ((g1 + g2) + g3) + g4 of four plain forward_backward calls with gscale = 1/8, and the
    update runs once, on the fourth call.  Against ONE batch of the same 8 images only the fp32
    summation order differs, so the bound is measured, not picked: d_ref is the largest per-tensor
    relative L2 difference between the one-batch gradient and the gradient of the same 8 images
    in permuted order, and the accumulated gradient must stay within 4 x d_ref of the one-batch
    gradient (4: the K = 4 extra fp32 roundings of the partial sums).
    Measured: d_ref = 5.56e-07 (conv2_block1_0_conv bias), accumulated vs one batch = 4.49e-07
    (conv2_block3_1_conv bias), i.e. 0.8 x d_ref against the bound of 4 x."""
    from pddl.parallel.strategies import make_strategy
    from pddl.train.trainer import Trainer
    img, lab, L = ref8["img"], ref8["lab"], ref8["L"]
    cfg = _cfg("single", batch_size=2, accum_steps=4)
    st = make_strategy(cfg)
    Trainer(cfg, st)
    assert torch.equal(st.engine.params, ref8["p0"])
    seen = []
    step = st.opt.step

    def spy():
        seen.append(st.engine.grads.clone())
        step()

    st.opt.step = spy
    for m in range(4):
        before = st.engine.params.clone()
        st.train_step(img[2 * m:2 * m + 2], lab[2 * m:2 * m + 2])
        assert len(seen) == (1 if m == 3 else 0)
        assert torch.equal(before, st.engine.params) == (m < 3)
    assert st.opt.iterations == 1
    e = _engine(2)
    want = None
    for m in range(4):
        e.forward_backward(img[2 * m:2 * m + 2], lab[2 * m:2 * m + 2], 1.0 / 8)
        want = e.grads.clone() if want is None else want + e.grads
    assert torch.equal(seen[0], want)
    d_acc, where = _per_tensor(L, seen[0], ref8["g_one"])
    print(f"d_ref = {ref8['d_ref']:.3e} ({ref8['where']}), accumulated vs one batch = {d_acc:.3e} ({where})")
    assert d_acc <= 4 * ref8["d_ref"], (d_acc, where, ref8["d_ref"])


def _rank_main(rank, world, port, kw, q, comm="bucket"):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port), LOCAL_WORLD_SIZE=str(world))
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import pddl  # noqa
    import torch.distributed as dist
    from pddl.parallel.strategies import HorovodStrategy
    from pddl.train.trainer import Trainer
    cfg = _cfg("horovod", **kw)
    st = HorovodStrategy(cfg, comm=comm)              # "bucket": the Python bucket reducer, whose calls can be counted
    tr = Trainer(cfg, st)
    calls, reduces = [], []
    if comm == "bucket":
        ready = st.reducer.on_bucket_ready
        st.reducer.on_bucket_ready = lambda i: (calls.append(i), ready(i))[1]
    else:
        assert type(st.fusion).__name__ == "FusionEngine"
    all_reduce = dist.all_reduce

    def counted(t, *a, **k):
        reduces.append(t.numel())
        return all_reduce(t, *a, **k)

    dist.all_reduce = counted
    tr.fit(1, [], validation=False)
    dist.all_reduce = all_reduce
    n = st.engine.L.n_trainable
    q.put((rank, st.engine.params[:n].numpy().copy(), calls, len(st.buckets), st.opt.iterations,
           [x for x in reduces if x > 8], st.engine.grads[:n].numpy().copy()))
    dist.barrier()
    dist.destroy_process_group()


def _spawn2(comm):
    from pddl.parallel.launch import pick_unused_port
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = pick_unused_port()
    kw = dict(batch_size=2, lr_scale_by_size=False, warmup_epochs=0, shard_by="batch", max_steps=2, accum_steps=2)
    ps = [ctx.Process(target=_rank_main, args=(r, 2, port, kw, q, comm)) for r in range(2)]
    for p in ps:
        p.start()
    out = sorted([q.get(timeout=600) for _ in range(2)], key=lambda t: t[0])
    for p in ps:
        p.join(timeout=60)
        assert p.exitcode == 0
    return out


def test_two_gloo_horovod_ranks_reduce_once_per_update(ref8):
    """2 ranks x batch 2 x K = 2: one update from 8 images, against the single-process step on the
    8 images as one batch.  SGD without momentum: the update is -lr x gradient, so the per-tensor
    bound measured for the gradient (4 x d_ref, `ref8`) bounds the parameters too (sharply for the
    zero-initialised biases and betas, where the parameter IS the update), and the all-reduced
    mean gradient itself is held to it as well.
    Measured: parameters 4.25e-07, mean gradient 4.23e-07 (both conv2_block3_1_conv bias) against
    d_ref = 5.56e-07."""
    from pddl.parallel.strategies import make_strategy
    from pddl.train.trainer import Trainer
    L, p0 = ref8["L"], ref8["p0"]
    cfg = _cfg("single", batch_size=8, max_steps=1)
    st = make_strategy(cfg)
    Trainer(cfg, st).fit(1, [], validation=False)
    n = L.n_trainable
    p_single = st.engine.params[:n].clone()
    assert torch.allclose(p_single, p0[:n] - LR * ref8["g_one"], rtol=1e-6, atol=1e-9)   # the same 8 images, one SGD step

    out = _spawn2("bucket")
    for rank, params, calls, nb, iters, reduces, grads in out:
        assert iters == 1
        assert calls == list(range(nb))               # every bucket once per UPDATE (two micro-steps ran)
        assert len(reduces) == nb                     # and one gradient all-reduce per bucket
        d, where = _per_tensor(L, torch.from_numpy(params), p_single)
        dg, whereg = _per_tensor(L, torch.from_numpy(grads), ref8["g_one"])
        print(f"rank {rank}: parameters vs single-process one batch = {d:.3e} ({where}), mean gradient = {dg:.3e} "
              f"({whereg}), d_ref = {ref8['d_ref']:.3e}")
        assert d <= 4 * ref8["d_ref"], (rank, d, where, ref8["d_ref"])
        assert dg <= 4 * ref8["d_ref"], (rank, dg, whereg, ref8["d_ref"])
    assert (out[0][1] == out[1][1]).all()
    # the native fusion engine (the default transport) applies the same sum: bit-identical parameters
    fus = _spawn2("fusion")
    assert (fus[0][1] == out[0][1]).all() and (fus[1][1] == out[0][1]).all()
    assert fus[0][4] == 1


def test_configuration_errors(capsys):
    from pddl import cli
    from pddl.config import config_from_args
    from pddl.parallel.strategies import make_strategy
    from pddl.train.trainer import Trainer
    for k in (0, -1):
        with pytest.raises(ValueError, match="accum-steps"):
            make_strategy(_cfg("single", batch_size=2, accum_steps=k))
    with pytest.raises(ValueError, match="--graphs"):
        make_strategy(_cfg("single", batch_size=2, accum_steps=2, graphs=True))
    with pytest.raises(ValueError, match="--bucket-mb"):
        make_strategy(_cfg("horovod", batch_size=2, accum_steps=2, bucket_mb=0.0))
    make_strategy(_cfg("single", batch_size=2, accum_steps=1, graphs=True))          # K = 1: as before
    # steps per epoch (after --max-steps) must be a multiple of K: raised before any step runs
    cfg = _cfg("single", batch_size=2, accum_steps=2, max_steps=3)
    st = make_strategy(cfg)
    tr = Trainer(cfg, st)
    ran = []
    st.train_step = lambda *a: ran.append(1)
    with pytest.raises(ValueError, match="multiple of --accum-steps"):
        tr.fit(1, [], validation=False)
    assert not ran
    # both spellings of the flag; the CLI reports configuration errors with exit status 2
    assert config_from_args("single", ["--accum-steps", "3"]).accum_steps == 3
    assert config_from_args("single", ["--backward-passes-per-step", "2"]).accum_steps == 2
    assert config_from_args("single", []).accum_steps == 1
    assert cli.run("single", ["--device", "cpu", "--accum-steps", "2", "--graphs"]) == 2
    assert "--graphs" in capsys.readouterr().err
    assert cli.run("ps", ["--device", "cpu", "--accum-steps", "2"]) == 2
    assert "--accum-steps is not supported for --strategy ps" in capsys.readouterr().err
    from pddl.parallel.parameter_server import run_ps_job
    with pytest.raises(ValueError, match="strategy ps"):
        run_ps_job(_cfg("ps", accum_steps=2))


def test_poly_schedule_counts_updates(tmp_path):
    """--lr-schedule poly is installed in updates (steps / K), optimizer.iterations advances once
    per update, and the epoch metrics keep counting micro-batches."""
    import json
    from pddl import cli
    jl = tmp_path / "m.jsonl"
    rc = cli.run("single", ["--device", "cpu", "--optimizer", "sgd", "--lr-schedule", "poly", "--warmup-epochs", "1",
                            "--lr", "0.05", "--lr-end", "0.002", "--batch-size", "2", "--crop", "32", "--image-size",
                            "32", "--validation-steps", "1", "--no-save", "--metrics-jsonl", str(jl), "--verbose", "0",
                            "--epochs", "2", "--steps-per-epoch", "4", "--accum-steps", "2"])
    assert rc == 0
    from pddl.train.optim import scheduled_lr
    recs = [json.loads(x) for x in jl.read_text().splitlines()]
    # 2 updates per epoch: warm-up ends at update 2, the schedule at update 4
    assert [r["lr"] for r in recs] == [scheduled_lr(0.05, t, 2, 4, 0.002) for t in (2, 4)] == [0.05, 0.002]
    assert all(r["accum_steps"] == 2 and r["effective_global_batch"] == 4 for r in recs)
