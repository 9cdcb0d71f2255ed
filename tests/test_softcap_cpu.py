"""Final-logit soft-capping on the CPU: the torch compositions behind
``softcap`` and ``cross_entropy_capped`` against the closed form in fp64, the
vocab-parallel option, and the wiring through ``ModelArgs``, ``Model.forward``,
the trainer, the exporter and the config."""
import json
import math
from pathlib import Path

import pytest
import torch

from mlx_cuda_distributed_pretraining_amd.core.config import Config
from mlx_cuda_distributed_pretraining_amd.core.trainer import Trainer
from mlx_cuda_distributed_pretraining_amd.models.llama import Model, ModelArgs, make_prompt_cache
from mlx_cuda_distributed_pretraining_amd.ops import (
    cross_entropy_capped,
    cross_entropy_ref,
    cross_entropy_with_z,
    softcap,
    softcap_,
)
from mlx_cuda_distributed_pretraining_amd.parallel.tp import vocab_parallel_cross_entropy

REPO = Path(__file__).resolve().parents[1]
IGN = -100


def _inputs(N, V, dtype, seed, mult=2.0):
    g = torch.Generator().manual_seed(seed)
    logits = (mult * torch.randn(N, V, generator=g)).to(dtype)
    tg = torch.randint(0, V, (N,), generator=g)
    tg[0], tg[1] = 0, V - 1
    tg[2::5] = IGN
    return logits, tg


# ---------------------------------- softcap ----------------------------------
def test_softcap_matches_the_closed_form_fp64():
    """c * (e^u - e^-u) / (e^u + e^-u), u = x / c, written out; t(0) = 0 and
    |t| <= c also far into saturation"""
    c = 3.0
    x = torch.tensor([0.0, 1e-9, -0.5, 0.5, 2.0, -7.0, 40.0, -1e4, 1e30], dtype=torch.float64)
    u = (x / c).clamp(-300, 300)
    want = c * (u.exp() - (-u).exp()) / (u.exp() + (-u).exp())
    got = softcap(x, c)
    assert got.dtype == torch.float64
    # e^u - e^-u cancels near 0: the written-out form is good to a few fp64
    # roundings of c in absolute terms there
    assert torch.allclose(got, want, rtol=1e-14, atol=8 * 2.0 ** -53 * c)
    assert float(got[0]) == 0.0 and bool((got.abs() <= c).all())
    assert float(got[-1]) == c and float(got[-2]) == -c
    # fp32 / bf16 input: fp32 math, the input's dtype out
    for dt in (torch.float32, torch.bfloat16):
        y = softcap(x.to(dt), c)
        assert y.dtype == dt
        assert torch.equal(y, (c * torch.tanh(x.to(dt).float() / c)).to(dt))


def test_softcap_gradcheck_fp64():
    g = torch.Generator().manual_seed(0)
    x = (3.0 * torch.randn(5, 7, generator=g, dtype=torch.float64)).requires_grad_(True)
    assert torch.autograd.gradcheck(lambda t: softcap(t, 2.5), (x,), eps=1e-6, atol=1e-8)
    y = softcap(x, 2.5)
    (gx,) = torch.autograd.grad(y.sum(), x)
    assert torch.allclose(gx, 1 - (y.detach() / 2.5) ** 2, rtol=1e-12, atol=1e-15)


def test_softcap_in_place_equals_out_of_place():
    x = torch.linspace(-50, 50, 41)
    want = softcap(x, 5.0)
    y = x.clone()
    assert softcap_(y, 5.0) is y
    assert torch.equal(y, want)
    nc = x.clone().reshape(1, 41).expand(2, 41).t()        # non-contiguous input
    assert torch.equal(softcap(nc, 5.0), want.reshape(1, 41).expand(2, 41).t())


@pytest.mark.parametrize("cap", [0.0, -1.0, float("nan"), float("inf")])
def test_ops_reject_a_bad_cap(cap):
    x, tg = _inputs(4, 8, torch.float32, seed=1)
    with pytest.raises(ValueError, match="cap"):
        softcap(x, cap)
    with pytest.raises(ValueError, match="cap"):
        softcap_(x.clone(), cap)
    with pytest.raises(ValueError, match="cap"):
        cross_entropy_capped(x, tg, cap, IGN)
    if cap != 0.0:      # 0 is "no cap" there
        with pytest.raises(ValueError, match="cap"):
            vocab_parallel_cross_entropy(x, tg, 0, IGN, softcap=cap)


# ---------------------------- cross_entropy_capped ---------------------------
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_capped_fallback_is_with_z_of_the_capped_logits(dtype):
    """values and gradients of 0.7 * ce + 0.3 * z, ignored rows included; the
    gradient also against the formula of the issue,
    (p * (a + b * lse) - a * onehot) * (1 - (t / c)^2)"""
    c = 2.0
    logits, tg = _inputs(23, 19, dtype, seed=2, mult=3.0)       # |x / c| up to ~5
    l1 = logits.clone().requires_grad_(True)
    ce, z, ntok = cross_entropy_capped(l1, tg, c, IGN)
    (0.7 * ce + 0.3 * z).backward()
    l2 = logits.double().requires_grad_(True)
    ce2, z2, ntok2 = cross_entropy_with_z(softcap(l2, c), tg, IGN)
    (0.7 * ce2 + 0.3 * z2).backward()
    tol = 1e-12 if dtype is torch.float64 else 1e-5
    assert int(ntok) == int(ntok2) == int((tg != IGN).sum())
    assert ce.dtype == dtype and l1.grad.dtype == dtype
    assert float(ce.detach()) == pytest.approx(float(ce2.detach()), rel=tol)
    assert float(z.detach()) == pytest.approx(float(z2.detach()), rel=tol)
    assert torch.allclose(l1.grad.double(), l2.grad, rtol=tol, atol=tol * float(l2.grad.abs().max()))
    assert not bool(l1.grad[tg == IGN].any()), "ignored rows are not exactly 0"

    t = c * torch.tanh(logits.double() / c)
    lse = torch.logsumexp(t, -1)
    n = int(ntok)
    a, b = 0.7 / n, 2 * 0.3 / n
    mask = (tg != IGN)[:, None]
    onehot = torch.zeros_like(t)
    rows = torch.nonzero(tg != IGN).squeeze(-1)
    onehot[rows, tg[rows]] = 1.0
    d = ((t - lse[:, None]).exp() * (a + b * lse)[:, None] - a * onehot) * (1 - (t / c) ** 2) * mask
    assert torch.allclose(l2.grad, d, rtol=1e-11, atol=1e-15)


def test_capped_fallback_gradcheck_and_all_ignored():
    logits, tg = _inputs(7, 11, torch.float64, seed=3)
    leaf = logits.clone().requires_grad_(True)
    assert torch.autograd.gradcheck(lambda x: cross_entropy_capped(x, tg, 1.5, IGN)[:2], (leaf,),
                                    eps=1e-6, atol=1e-7)
    none = torch.full_like(tg, IGN)
    ce, z, ntok = cross_entropy_capped(leaf, none, 1.5, IGN)
    (ce + 0.5 * z).backward()
    assert float(ce.detach()) == 0.0 and float(z.detach()) == 0.0 and int(ntok) == 0
    assert not bool(leaf.grad.any())


def test_a_large_cap_approaches_the_plain_loss():
    logits, tg = _inputs(16, 24, torch.float64, seed=4)
    ce, _, _ = cross_entropy_capped(logits, tg, 1e6, IGN)
    plain, _ = cross_entropy_ref(logits.float(), tg, IGN)
    assert float(ce) == pytest.approx(float(plain), rel=1e-5)
    capped, _, _ = cross_entropy_capped(logits, tg, 1.0, IGN)
    assert abs(float(capped) - float(plain)) > 0.05, "cap 1 must change this loss"


# ------------------------------- vocab-parallel ------------------------------
def test_vocab_parallel_softcap_world1_equals_the_unsharded_op():
    c = 2.0
    logits, tg = _inputs(21, 16, torch.float32, seed=5, mult=3.0)
    l1 = logits.clone().requires_grad_(True)
    ce1, z1, n1 = cross_entropy_capped(l1, tg, c, IGN)
    (ce1 + 0.1 * z1).backward()
    l2 = logits.clone().requires_grad_(True)
    out = vocab_parallel_cross_entropy(l2, tg, 0, IGN, with_z=True, softcap=c)
    assert len(out) == 3
    ce2, z2, n2 = out
    (ce2 + 0.1 * z2).backward()
    assert int(n1) == int(n2)
    assert float(ce2.detach()) == pytest.approx(float(ce1.detach()), rel=1e-6)
    assert float(z2.detach()) == pytest.approx(float(z1.detach()), rel=1e-6)
    assert torch.allclose(l1.grad, l2.grad, rtol=1e-5, atol=1e-8)
    two = vocab_parallel_cross_entropy(logits, tg, 0, IGN, softcap=c)
    assert len(two) == 2 and torch.equal(two[0], ce2.detach())


def test_vocab_parallel_softcap_zero_is_the_uncapped_function():
    """softcap = 0 (the default) returns what the function returned before the
    option existed: the same values with and without the argument, and the
    loss of cross_entropy_ref"""
    logits, tg = _inputs(21, 16, torch.float32, seed=6)
    l0 = logits.clone().requires_grad_(True)
    base = vocab_parallel_cross_entropy(l0, tg, 0, IGN)
    base[0].backward()
    l1 = logits.clone().requires_grad_(True)
    zero = vocab_parallel_cross_entropy(l1, tg, 0, IGN, softcap=0.0)
    zero[0].backward()
    assert len(base) == len(zero) == 2
    assert torch.equal(base[0], zero[0]) and torch.equal(base[1], zero[1])
    assert torch.equal(l0.grad, l1.grad)
    ref, ntok = cross_entropy_ref(logits, tg, IGN)
    assert int(base[1]) == int(ntok)
    assert float(base[0].detach()) == pytest.approx(float(ref), rel=1e-6)
    z0 = vocab_parallel_cross_entropy(logits, tg, 0, IGN, with_z=True)
    z1 = vocab_parallel_cross_entropy(logits, tg, 0, IGN, with_z=True, softcap=0.0)
    assert len(z0) == 3 and all(torch.equal(x, y) for x, y in zip(z0, z1))


# ------------------------------ ModelArgs, Model -----------------------------
def tiny_args(**kw):
    defaults = dict(hidden_size=64, intermediate_size=128, num_layers=2, num_heads=4,
                    num_kv_heads=2, vocab_size=101)
    defaults.update(kw)
    return ModelArgs(**defaults)


def test_model_args_validation():
    assert tiny_args().logit_softcap is None
    assert tiny_args(logit_softcap=None).logit_softcap is None
    assert tiny_args(logit_softcap=0).logit_softcap is None
    assert tiny_args(logit_softcap=0.0).logit_softcap is None
    assert tiny_args(logit_softcap=30).logit_softcap == 30.0
    for bad in (-1.0, float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError, match="logit_softcap"):
            tiny_args(logit_softcap=bad)


def _tiny_model(**kw):
    torch.manual_seed(0)
    return Model(tiny_args(**kw)).eval()


def test_model_caps_after_logit_scale_and_cap_logits_false_is_raw():
    c = 1.5
    m = _tiny_model(logit_softcap=c, logit_scale=8.0)
    plain = _tiny_model(logit_scale=8.0)
    x = torch.randint(0, 101, (2, 9), generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        raw = m(x, cap_logits=False)
        capped = m(x)
        assert torch.equal(raw, plain(x)), "cap_logits=False must be the uncapped model"
        assert torch.equal(plain(x, cap_logits=False), plain(x))
    assert float(raw.abs().max()) > 2 * c, "the test wants saturating logits"
    assert torch.equal(capped, c * torch.tanh(raw / c))
    assert float(capped.abs().max()) <= c


def test_model_without_the_key_is_unchanged():
    """a config that never mentions logit_softcap and one with it off build
    the same model: torch.equal logits, and softcap is never called"""
    cfg = Config.from_yaml(str(REPO / "configs" / "model-config-sample.yaml"))
    assert "logit_softcap" not in (cfg.model.misc or {})
    a0 = ModelArgs.from_config(cfg.model, 101)
    assert a0.logit_softcap is None
    cfg.model.misc = dict(cfg.model.misc or {}, logit_softcap=0)
    a1 = ModelArgs.from_config(cfg.model, 101)
    assert a1.logit_softcap is None
    cfg.model.misc["logit_softcap"] = 7.5
    assert ModelArgs.from_config(cfg.model, 101).logit_softcap == 7.5
    x = torch.randint(0, 101, (2, 9), generator=torch.Generator().manual_seed(2))
    outs = []
    for a in (a0, a1):
        torch.manual_seed(0)
        with torch.no_grad():
            outs.append(Model(a).eval()(x))
    assert torch.equal(outs[0], outs[1])


def test_cached_path_returns_capped_logits():
    c = 1.5
    m = _tiny_model(logit_softcap=c, logit_scale=8.0)
    x = torch.randint(0, 101, (1, 9), generator=torch.Generator().manual_seed(3))
    with torch.no_grad():
        full = m(x)
        cache = make_prompt_cache(m)
        m(x[:, :-1], cache=cache)
        last = m(x[:, -1:], cache=cache)
        raw_last = None
        cache2 = make_prompt_cache(m)
        m(x[:, :-1], cache=cache2)
        raw_last = m(x[:, -1:], cache=cache2, cap_logits=False)
    assert float(last.abs().max()) <= c
    assert torch.allclose(last[:, -1], full[:, -1], rtol=0, atol=1e-5)
    assert torch.equal(last, c * torch.tanh(raw_last / c))
    assert float(raw_last.abs().max()) > c


def test_static_decoder_on_cpu_follows_the_capped_model():
    from mlx_cuda_distributed_pretraining_amd.inference.generate import generate_step
    from mlx_cuda_distributed_pretraining_amd.inference.static_decode import GraphDecoder

    torch.manual_seed(0)
    m = Model(ModelArgs(hidden_size=64, intermediate_size=128, num_layers=2, num_heads=4,
                        num_kv_heads=2, head_dim=16, vocab_size=97, logit_softcap=1.5,
                        logit_scale=8.0)).eval()
    prompt = [1, 2, 3, 4, 5]
    oracle = list(generate_step(m, prompt, max_tokens=6))
    dec = GraphDecoder(m, batch=1, max_len=64)
    dec.prefill(torch.tensor([prompt]))
    assert dec.decode(6)[0].tolist() == oracle


# ---------------------------------- trainer ----------------------------------
def _cfg(name, cap=None, **hp):
    cfg = Config.from_yaml(str(REPO / "configs" / "model-config-sample.yaml"))
    cfg.name = name
    cfg.model.dimensions = {"hidden_size": 32, "intermediate_size": 64, "num_layers": 2}
    cfg.model.attention = {"num_heads": 2, "num_kv_heads": None, "head_dim": None,
                           "max_position_embeddings": None}
    cfg.model.misc = dict(cfg.model.misc or {}, logit_scale=40.0)
    if cap is not None:
        cfg.model.misc["logit_softcap"] = cap
    cfg.data.preprocessing["max_context_size"] = 32
    cfg.training.hyperparameters["batch_size"] = 4
    cfg.training.hyperparameters["iters"] = 2
    cfg.training.hyperparameters.update(hp)
    cfg.logging.steps = {"logging_interval": 1, "checkpoint_interval": 0,
                         "validation_interval": 0}
    return cfg


def _manual(t, inputs, targets, cap):
    """fp64 (ce, z) of the capped logits of the trainer's model on one batch"""
    with torch.no_grad():
        raw = t.model(inputs, cap_logits=False).reshape(-1, t.model_args.vocab_size).double()
    tl = cap * torch.tanh(raw / cap) if cap else raw
    tg = targets.reshape(-1)
    mask = tg != t.tokenizer.PAD_TOKEN
    lse = torch.logsumexp(tl, -1)
    picked = tl.gather(-1, tg.clamp_min(0)[:, None]).squeeze(-1)
    n = mask.sum()
    return (float(((lse - picked) * mask).sum() / n), float((lse * lse * mask).sum() / n),
            float(raw.abs().max()))


def test_trainer_takes_the_capped_loss_in_training_and_validation(tmp_runs, monkeypatch):
    from mlx_cuda_distributed_pretraining_amd.core import trainer as trainer_mod

    cap = 2.0
    t = Trainer(_cfg("cap-on", cap=cap), runs_root=tmp_runs)
    assert t.model_args.logit_softcap == cap and t.z_loss_coef == 0.0
    calls = []
    real = trainer_mod.cross_entropy_capped
    monkeypatch.setattr(trainer_mod, "cross_entropy_capped",
                        lambda *a, **k: (calls.append(a[2]), real(*a, **k))[1])
    monkeypatch.setattr(trainer_mod, "fused_cross_entropy",
                        lambda *a, **k: pytest.fail("the plain loss ran with a cap configured"))
    batch = t.data_manager.generate_batch(0)
    inputs, targets = batch[:, :-1], batch[:, 1:]
    ce, z, raw_max = _manual(t, inputs, targets, cap)
    ce_raw, _, _ = _manual(t, inputs, targets, None)
    assert raw_max > 2 * cap and abs(ce - ce_raw) > 1e-2, "the cap must matter on this batch"

    t.model.train()
    loss, _ = t.compute_loss(inputs, targets)
    assert float(loss.detach()) == pytest.approx(ce, rel=1e-5)
    t.model.eval()
    with torch.no_grad():
        loss_eval, _ = t.compute_loss(inputs, targets)
    assert float(loss_eval.detach()) == pytest.approx(ce, rel=1e-5)   # validation is capped too
    t.model.train()
    step_loss, _ = t.train_step(0)
    assert float(step_loss.detach()) == pytest.approx(ce, rel=1e-5)
    assert t.last_z_loss is None                                     # no z without a coefficient
    assert calls == [cap] * 3


def test_trainer_adds_z_of_the_capped_logits_only_with_a_coefficient(tmp_runs):
    cap, coef = 2.0, 0.05
    t = Trainer(_cfg("cap-z", cap=cap, z_loss_coef=coef), runs_root=tmp_runs)
    batch = t.data_manager.generate_batch(0)
    inputs, targets = batch[:, :-1], batch[:, 1:]
    ce, z, _ = _manual(t, inputs, targets, cap)
    assert coef * z > 1e-3 * ce
    t.model.train()
    loss, _ = t.compute_loss(inputs, targets)
    assert float(loss.detach()) == pytest.approx(ce + coef * z, rel=1e-5)
    assert float(t._z_micro) == pytest.approx(z, rel=1e-5)
    t.model.eval()
    with torch.no_grad():
        loss_eval, _ = t.compute_loss(inputs, targets)
    assert float(loss_eval.detach()) == pytest.approx(ce, rel=1e-5)   # z only in training
    t.model.train()


def test_trainer_without_a_cap_never_calls_the_capped_loss(tmp_runs, monkeypatch):
    from mlx_cuda_distributed_pretraining_amd.core import trainer as trainer_mod

    monkeypatch.setattr(trainer_mod, "cross_entropy_capped",
                        lambda *a, **k: pytest.fail("the capped loss ran without a cap"))
    runs = []
    for name, c in (("cap-absent", None), ("cap-zero", 0)):
        t = Trainer(_cfg(name, cap=c), runs_root=tmp_runs)
        loss, ntok = t.train_step(0)
        runs.append((loss.clone(), {n: p.grad.clone() for n, p in t.model.named_parameters()}))
    assert torch.equal(runs[0][0], runs[1][0])
    for n in runs[0][1]:
        assert torch.equal(runs[0][1][n], runs[1][1][n]), n


# ------------------------------ exporter, config -----------------------------
def test_exporter_refuses_a_capped_model(tmp_path):
    import sys

    sys.path.insert(0, str(REPO / "tools"))
    import convert_to_mlx_lm as conv

    cfg = _cfg("cap-export", cap=30.0)
    args = ModelArgs.from_config(cfg.model, 259)
    with pytest.raises(NotImplementedError, match="logit_softcap"):
        conv.hf_config_from(cfg, args)
    run = tmp_path / "run"
    run.mkdir()
    cfg.save_yaml(run / "config.yaml")
    with pytest.raises(NotImplementedError, match="logit_softcap"):
        conv.convert_run(run, tmp_path / "out")
    assert not (tmp_path / "out" / "config.json").exists()
    assert not (tmp_path / "out" / "model.safetensors").exists()
    ok = conv.hf_config_from(_cfg("cap-export-off"), ModelArgs.from_config(_cfg("x").model, 259))
    assert json.dumps(ok) and "logit_softcap" not in ok


def test_softcap_config_extends_the_qk_norm_config():
    cfg = Config.from_yaml(str(REPO / "configs" / "model-config-400m-muon-qknorm-softcap.yaml"))
    base = Config.from_yaml(str(REPO / "configs" / "model-config-400m-muon-qknorm.yaml"))
    assert cfg.model.misc["logit_softcap"] == 30.0
    assert "logit_softcap" not in base.model.misc
    assert {k: v for k, v in cfg.model.misc.items() if k != "logit_softcap"} == base.model.misc
    assert cfg.model.attention["qk_norm"] is True and cfg.model.dimensions == base.model.dimensions
    assert ModelArgs.from_config(cfg.model, 32000).logit_softcap == 30.0
    assert math.isclose(cfg.training.hyperparameters["learning_rate"],
                        base.training.hyperparameters["learning_rate"])
