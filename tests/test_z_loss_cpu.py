"""Auxiliary z-loss on the CPU: the torch composition behind
``cross_entropy_with_z`` against an fp64 closed form and gradcheck, the
vocab-parallel variant on two gloo ranks against the full-vocab result, and
the trainer wiring (objective, evaluation, log line, the zero coefficient)."""
import os
import re
from pathlib import Path

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from mlx_cuda_distributed_pretraining_amd.core.config import Config
from mlx_cuda_distributed_pretraining_amd.core.trainer import Trainer
from mlx_cuda_distributed_pretraining_amd.ops import cross_entropy_with_z, fused_cross_entropy

REPO = Path(__file__).resolve().parents[1]
IGN = -100


def _inputs(N, V, dtype, seed, all_ignored=False):
    g = torch.Generator().manual_seed(seed)
    logits = (2.0 * torch.randn(N, V, generator=g)).to(dtype)
    tg = torch.randint(0, V, (N,), generator=g)
    tg[0], tg[1] = 0, V - 1
    tg[2::5] = IGN
    if all_ignored:
        tg[:] = IGN
    return logits, tg


def _closed_form(logits, tg, g_ce, g_z):
    """fp64 (ce, z, dlogits) written out from the definitions: a loop over the
    rows, no logsumexp and no autograd"""
    l = logits.double()
    N, V = l.shape
    counted = [i for i in range(N) if int(tg[i]) != IGN]
    ntok = max(len(counted), 1)
    ce = z = 0.0
    d = torch.zeros_like(l)
    a, b = g_ce / ntok, 2.0 * g_z / ntok
    for i in counted:
        lse = float(torch.log(torch.exp(l[i] - l[i].max()).sum()) + l[i].max())
        ce += lse - float(l[i, tg[i]])
        z += lse * lse
        d[i] = torch.exp(l[i] - lse) * (a + b * lse)
        d[i, tg[i]] -= a
    return ce / ntok, z / ntok, d, len(counted)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_fallback_matches_closed_form(dtype):
    """means and gradient of 0.7*ce + 0.3*z; fp64 inputs at fp64 accuracy,
    fp32 inputs (taken as stored) at a few fp32 roundings of the values"""
    logits, tg = _inputs(23, 19, dtype, seed=1)      # V % 8 != 0, rows 2, 7, .. ignored
    leaf = logits.clone().requires_grad_(True)
    ce, z, ntok = cross_entropy_with_z(leaf, tg, IGN)
    (0.7 * ce + 0.3 * z).backward()
    ce_r, z_r, d_r, n_r = _closed_form(logits, tg, 0.7, 0.3)
    tol = 1e-12 if dtype is torch.float64 else 1e-5
    assert int(ntok) == n_r and n_r < 23
    assert ce.dtype == dtype and leaf.grad.dtype == dtype
    assert float(ce.detach()) == pytest.approx(ce_r, rel=tol)
    assert float(z.detach()) == pytest.approx(z_r, rel=tol)
    assert torch.allclose(leaf.grad.double(), d_r, rtol=tol, atol=tol * float(d_r.abs().max()))
    assert not bool(leaf.grad[tg == IGN].any()), "ignored rows are not exactly 0"
    # each counted row sums to b * lse_i
    lse = torch.logsumexp(logits.double(), -1)
    want = torch.where(tg != IGN, 2 * 0.3 / n_r * lse, torch.zeros_like(lse))
    assert torch.allclose(leaf.grad.double().sum(-1), want, atol=tol * 10)


def test_fallback_gradcheck_fp64():
    logits, tg = _inputs(7, 11, torch.float64, seed=2)
    leaf = logits.clone().requires_grad_(True)

    def f(x):
        ce, z, _ = cross_entropy_with_z(x, tg, IGN)
        return 0.6 * ce + 0.05 * z      # both outputs feed the loss

    assert torch.autograd.gradcheck(f, (leaf,), eps=1e-6, atol=1e-7)
    assert torch.autograd.gradcheck(lambda x: cross_entropy_with_z(x, tg, IGN)[:2], (leaf,),
                                    eps=1e-6, atol=1e-7)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_fallback_all_targets_ignored(dtype):
    logits, tg = _inputs(9, 16, dtype, seed=3, all_ignored=True)
    leaf = logits.clone().requires_grad_(True)
    ce, z, ntok = cross_entropy_with_z(leaf, tg, IGN)
    (ce + 0.5 * z).backward()
    assert float(ce.detach()) == 0.0 and float(z.detach()) == 0.0 and int(ntok) == 0
    assert not bool(leaf.grad.any()) and bool(torch.isfinite(leaf.grad).all())


def test_zero_z_gradient_gives_the_plain_ce_gradient():
    """(ce + 0*z).backward() against fused_cross_entropy on the same inputs:
    the z term adds exact zeros, the CE terms differ by the order of two fp32
    roundings at most (softmax*s - onehot*s against (softmax - onehot)*s)"""
    logits, tg = _inputs(23, 40, torch.float32, seed=4)
    l1 = logits.clone().requires_grad_(True)
    ce, z, ntok = cross_entropy_with_z(l1, tg, IGN)
    (ce + 0.0 * z).backward()
    l2 = logits.clone().requires_grad_(True)
    loss, ntok2 = fused_cross_entropy(l2, tg, IGN)
    loss.backward()
    assert int(ntok) == int(ntok2)
    assert float(ce.detach()) == pytest.approx(float(loss.detach()), rel=1e-6)
    scale = 1.0 / int(ntok)
    assert torch.allclose(l1.grad, l2.grad, rtol=0, atol=4 * 2.0 ** -24 * scale)
    assert not bool(l1.grad[tg == IGN].any())


# ------------------------- vocab-parallel, 2 gloo ranks ----------------------
def _free_port():
    import socket

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


VP_N, VP_V = 21, 24


def _vp_worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from mlx_cuda_distributed_pretraining_amd.parallel.tp import vocab_parallel_cross_entropy

        logits, tg = _inputs(VP_N, VP_V, torch.float32, seed=5)
        half = VP_V // world
        shard = logits[:, rank * half:(rank + 1) * half].clone().requires_grad_(True)
        ce, z, ntok = vocab_parallel_cross_entropy(shard, tg, rank * half, IGN, with_z=True)
        (0.7 * ce + 0.3 * z).backward()
        plain, ntok_p = vocab_parallel_cross_entropy(shard.detach(), tg, rank * half, IGN)
        q.put({"rank": rank, "ce": float(ce.detach()), "z": float(z.detach()),
               "ntok": int(ntok),
               "plain": float(plain), "ntok_plain": int(ntok_p),
               "grad": shard.grad.numpy().copy()})
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(240)
def test_vocab_parallel_with_z_matches_full_vocab_on_2_ranks():
    logits, tg = _inputs(VP_N, VP_V, torch.float32, seed=5)
    leaf = logits.clone().requires_grad_(True)
    ce, z, ntok = cross_entropy_with_z(leaf, tg, IGN)
    (0.7 * ce + 0.3 * z).backward()

    ctx = mp.get_context("spawn")
    q = ctx.SimpleQueue()
    port = _free_port()
    procs = [ctx.Process(target=_vp_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(), q.get()]
    for p in procs:
        p.join(180)
        assert p.exitcode == 0
    half = VP_V // 2
    for r in res:
        rk = r["rank"]
        assert r["ntok"] == int(ntok) == r["ntok_plain"]
        assert r["ce"] == pytest.approx(float(ce.detach()), rel=1e-5)
        assert r["z"] == pytest.approx(float(z.detach()), rel=1e-5)
        # with_z=False still returns (loss, ntok)
        assert r["plain"] == pytest.approx(float(ce.detach()), rel=1e-5)
        assert torch.allclose(torch.from_numpy(r["grad"]),
                              leaf.grad[:, rk * half:(rk + 1) * half], atol=1e-6)


# ----------------------- sequence-parallel trainer, 2 ranks ------------------
SP_COEF = 0.05


def _sp_cfg(name, system):
    return Config.from_dict({
        "name": name,
        "overwrite": True,
        "data": {"synthetic": True, "synthetic_vocab_size": 64,
                 "preprocessing": {"max_context_size": 33}},  # 32 after the shift
        "model": {"dimensions": {"hidden_size": 32, "intermediate_size": 64, "num_layers": 2},
                  "attention": {"num_heads": 4, "num_kv_heads": 2,
                                "max_position_embeddings": 64}},
        "training": {"hyperparameters": {"iters": 2, "batch_size": 2, "learning_rate": 1e-3,
                                         "z_loss_coef": SP_COEF}},
        "logging": {"steps": {"logging_interval": 0, "checkpoint_interval": 0,
                              "validation_interval": 0}},
        "system": dict({"device": "cpu"}, **system),
    })


def _sp_worker(rank, world, port, q, runs_root):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ["RANK"] = str(rank)
    os.environ["WORLD_SIZE"] = str(world)
    os.environ["LOCAL_RANK"] = str(rank)
    try:
        t = Trainer(_sp_cfg("z-sp", {"distributed": True, "distributed_backend": "gloo",
                                     "model_parallel": True, "model_parallel_size": 2,
                                     "sequence_parallel": True}),
                    runs_root=f"{runs_root}{rank}")
        out = []
        for i in range(2):
            loss, _ = t.train_step(i)
            out.append((float(loss.detach()), float(t.last_z_loss)))
        q.put({"rank": rank, "steps": out})
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_sequence_parallel_z_loss_matches_single_process(tmp_path):
    """TP=2 + sequence parallelism with z_loss_coef > 0: each rank holds half
    of every sequence, and the objective and the raw z of every step equal the
    single-process trainer's (same data, same seed)."""
    ref_t = Trainer(_sp_cfg("z-sp-ref", {}), runs_root=str(tmp_path / "ref"))
    ref = []
    for i in range(2):
        loss, _ = ref_t.train_step(i)
        ref.append((float(loss.detach()), float(ref_t.last_z_loss)))
    assert SP_COEF * ref[0][1] > 1e-3 * ref[0][0], "the z term is too small to be seen"

    ctx = mp.get_context("spawn")
    q = ctx.SimpleQueue()
    port = _free_port()
    procs = [ctx.Process(target=_sp_worker, args=(r, 2, port, q, str(tmp_path / "sp")))
             for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(), q.get()]
    for p in procs:
        p.join(240)
        assert p.exitcode == 0
    for r in res:
        for (loss, z), (loss_r, z_r) in zip(r["steps"], ref):
            assert loss == pytest.approx(loss_r, abs=2e-5)
            assert z == pytest.approx(z_r, rel=1e-5)


# --------------------------------- trainer -----------------------------------
def _cfg(name, **hp):
    cfg = Config.from_yaml(str(REPO / "configs" / "model-config-sample.yaml"))
    cfg.name = name
    cfg.model.dimensions = {"hidden_size": 32, "intermediate_size": 64, "num_layers": 2}
    cfg.model.attention = {"num_heads": 2, "num_kv_heads": None, "head_dim": None,
                           "max_position_embeddings": None}
    cfg.data.preprocessing["max_context_size"] = 32
    cfg.training.hyperparameters["batch_size"] = 4
    cfg.training.hyperparameters["iters"] = 2
    cfg.training.hyperparameters.update(hp)
    cfg.logging.steps = {"logging_interval": 1, "checkpoint_interval": 0,
                         "validation_interval": 0}
    return cfg


def test_trainer_objective_is_ce_plus_coef_z_and_eval_is_pure_ce(tmp_runs):
    coef = 0.05
    t = Trainer(_cfg("z-on", z_loss_coef=coef), runs_root=tmp_runs)
    assert t.z_loss_coef == coef
    batch = t.data_manager.generate_batch(0)
    inputs, targets = batch[:, :-1], batch[:, 1:]
    pad = t.tokenizer.PAD_TOKEN

    with torch.no_grad():
        logits = t.model(inputs).reshape(-1, t.model_args.vocab_size).double()
    tg = targets.reshape(-1)
    mask = tg != pad
    lse = torch.logsumexp(logits, -1)
    picked = logits.gather(-1, tg.clamp_min(0)[:, None]).squeeze(-1)
    ce = float(((lse - picked) * mask).sum() / mask.sum())
    z = float((lse * lse * mask).sum() / mask.sum())

    t.model.train()
    loss, ntok = t.compute_loss(inputs, targets)
    assert int(ntok) == int(mask.sum())
    assert float(loss.detach()) == pytest.approx(ce + coef * z, rel=1e-5)
    assert float(t._z_micro) == pytest.approx(z, rel=1e-5)
    assert coef * z > 1e-3 * ce, "the z term is too small for this test to see it"

    t.model.eval()
    with torch.no_grad():
        loss_eval, _ = t.compute_loss(inputs, targets)
    assert float(loss_eval.detach()) == pytest.approx(ce, rel=1e-5)
    t.model.train()

    step_loss, _ = t.train_step(0)
    assert float(step_loss.detach()) == pytest.approx(ce + coef * z, rel=1e-5)
    assert float(t.last_z_loss) == pytest.approx(z, rel=1e-5)


def test_log_line_carries_z_loss_only_with_a_positive_coefficient(tmp_runs):
    field = re.compile(r"^.*Step \d+: .*loss=.*\| z_loss=\d\.\d{4}e[+-]\d+$", re.M)
    on = _cfg("z-log-on", z_loss_coef=1e-3)
    Trainer(on, runs_root=tmp_runs).train()
    log = (Path(tmp_runs) / on.name / "log.txt").read_text()
    assert len(field.findall(log)) == 2, log

    for name, hp in (("z-log-off", {}), ("z-log-zero", {"z_loss_coef": 0.0})):
        off = _cfg(name, **hp)
        Trainer(off, runs_root=tmp_runs).train()
        log = (Path(tmp_runs) / off.name / "log.txt").read_text()
        assert re.search(r"Step \d+: .*loss=", log) and "z_loss" not in log, log


def test_z_loss_config_extends_the_qk_norm_config():
    cfg = Config.from_yaml(str(REPO / "configs" / "model-config-400m-muon-qknorm-zloss.yaml"))
    base = Config.from_yaml(str(REPO / "configs" / "model-config-400m-muon-qknorm.yaml"))
    assert cfg.training.hyperparameters["z_loss_coef"] == 1.0e-4
    assert "z_loss_coef" not in base.training.hyperparameters
    assert cfg.model.attention["qk_norm"] is True
    assert cfg.model.dimensions == base.model.dimensions


def test_negative_coefficient_is_rejected(tmp_runs):
    with pytest.raises(ValueError, match="z_loss_coef"):
        Trainer(_cfg("z-neg", z_loss_coef=-1e-4), runs_root=tmp_runs)


def test_zero_coefficient_is_bit_identical_to_no_key(tmp_runs):
    """z_loss_coef: 0 takes the plain calls: loss and every parameter
    gradient of one train_step equal a trainer built without the key"""
    runs = []
    for name, hp in (("z-absent", {}), ("z-zero", {"z_loss_coef": 0})):
        t = Trainer(_cfg(name, **hp), runs_root=tmp_runs)
        loss, ntok = t.train_step(0)
        runs.append((loss.clone(), int(ntok),
                     {n: p.grad.clone() for n, p in t.model.named_parameters()}))
        assert t.last_z_loss is None
    (l0, n0, g0), (l1, n1, g1) = runs
    assert n0 == n1 and torch.equal(l0, l1)
    assert g0.keys() == g1.keys() and len(g0) > 0
    for n in g0:
        assert torch.equal(g0[n], g1[n]), n
