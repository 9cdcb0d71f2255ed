"""Fused per-head QK-norm + RoPE on a real MI355X: the qknorm_rope kernels
(csrc/qknorm_rope.hip) behind ops.qk_norm_rope, rope_flash_attention_qkv(
q_norm_weight=..., k_norm_weight=...), Model(qk_norm=True) and the static
decode path, against the fp32 composition rms_norm_ref -> rope_ref on fp32
leaves built from the same bf16 inputs. Tolerances are the project's own
(tests/test_gpu_doc_mask.py): forward max abs error < 3e-2, each gradient
(dw included) < 0.05 * max(max|ref|, 1); rstd relative error < 1e-5."""
import math

import pytest
import torch

from test_qk_norm_cpu import _randomize_norms, qknorm_rope_backward_formula

pytestmark = pytest.mark.gpu

EPS = 1e-5


def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ext():
    from mlx_cuda_distributed_pretraining_amd.ops import require_ext

    return require_ext()


def _check(name, got, want):
    assert bool(torch.isfinite(got).all()), f"{name} has non-finite values"
    err = (got.float() - want.float()).abs().max().item()
    bound = 0.05 * max(want.abs().max().item(), 1.0)
    print(f"{name}: max abs err {err:.4g} (bound {bound:.4g})")
    assert math.isfinite(err) and err < bound, f"{name} err {err} >= {bound}"


def _check_fwd(name, got, want):
    assert bool(torch.isfinite(got).all()), f"{name} has non-finite values"
    err = (got.detach().float() - want.detach().float()).abs().max().item()
    print(f"{name}: max abs err {err:.4g}")
    assert math.isfinite(err) and err < 3e-2, f"{name} forward err {err}"


def _weights(g, D, dtype=torch.bfloat16):
    """random in roughly [0.5, 1.5]: a dropped `* w` must not go unnoticed"""
    mk = lambda: (0.5 + torch.rand(D, generator=g)).to(dev(), dtype)  # noqa: E731
    return mk(), mk()


def _fused_qkv(g, B, S, Hq, Hkv, D):
    return torch.randn(B, S, (Hq + 2 * Hkv) * D, generator=g).to(dev(), torch.bfloat16)


def _views(qkv, Hq, Hkv, D):
    B, S, _ = qkv.shape
    q, k, v = qkv.split([Hq * D, Hkv * D, Hkv * D], dim=-1)
    return q.view(B, S, Hq, D), k.view(B, S, Hkv, D), v.view(B, S, Hkv, D)


def _oracle(x, w, cos, sin, traditional, offset):
    """fp32 composition on fp32 tensors"""
    from mlx_cuda_distributed_pretraining_amd.ops.rmsnorm import rms_norm_ref
    from mlx_cuda_distributed_pretraining_amd.ops.rope import rope_ref

    return rope_ref(rms_norm_ref(x, w, EPS), cos, sin, traditional, offset)


def _leaf(t):
    return t.detach().float().requires_grad_(True)


def _run_op_case(ext, B, S, Hq, Hkv, D, traditional, offset, seed=31, on_device_rng=False):
    from mlx_cuda_distributed_pretraining_amd.ops import qk_norm_rope
    from mlx_cuda_distributed_pretraining_amd.ops.rope import RopeTable

    g = torch.Generator(device="cpu").manual_seed(seed)
    if on_device_rng:  # the large case: keep the host out of it
        gd = torch.Generator(device=dev()).manual_seed(seed)
        qkv = torch.randn(B, S, (Hq + 2 * Hkv) * D, generator=gd, device=dev(),
                          dtype=torch.bfloat16)
        gq = torch.randn(B, S, Hq, D, generator=gd, device=dev(), dtype=torch.bfloat16)
        gk = torch.randn(B, S, Hkv, D, generator=gd, device=dev(), dtype=torch.bfloat16)
    else:
        qkv = _fused_qkv(g, B, S, Hq, Hkv, D)
        gq = torch.randn(B, S, Hq, D, generator=g).to(dev(), torch.bfloat16)
        gk = torch.randn(B, S, Hkv, D, generator=g).to(dev(), torch.bfloat16)
    wq, wk = _weights(g, D)
    cos, sin = RopeTable(D, 10000.0).get(S, dev(), offset)

    qkv.requires_grad_(True)
    wq.requires_grad_(True)
    wk.requires_grad_(True)
    q, k, _ = _views(qkv, Hq, Hkv, D)  # strided views of ONE fused tensor
    assert not q.is_contiguous() and not k.is_contiguous()
    qo, ko = qk_norm_rope(q, k, wq, wk, cos, sin, EPS, traditional=traditional, offset=offset)
    assert type(qo.grad_fn).__name__ == "_QKNormRopeFnBackward"
    torch.autograd.backward([qo, ko], [gq, gk])

    qkv_f, wq_f, wk_f = _leaf(qkv), _leaf(wq), _leaf(wk)
    qf, kf, _ = _views(qkv_f, Hq, Hkv, D)
    qo_ref = _oracle(qf, wq_f, cos, sin, traditional, offset)
    ko_ref = _oracle(kf, wk_f, cos, sin, traditional, offset)
    torch.autograd.backward([qo_ref, ko_ref], [gq.float(), gk.float()])

    _check_fwd("q'", qo, qo_ref)
    _check_fwd("k'", ko, ko_ref)
    # v's slice of the fused grad gets no contribution here
    n_qk = (Hq + Hkv) * D
    _check("dq|dk", qkv.grad[..., :n_qk], qkv_f.grad[..., :n_qk])
    _check("dw_q", wq.grad, wq_f.grad)
    _check("dw_k", wk.grad, wk_f.grad)
    # the analytical backward (tests/test_qk_norm_cpu.py) is what the kernel
    # computes: same bound against it, evaluated in fp32 on the same inputs
    dq_f, dwq_f, _ = qknorm_rope_backward_formula(gq.float(), qf.detach(), wq_f.detach(),
                                                  cos, sin, EPS, traditional, offset)
    _check("dq vs formula", qkv.grad[..., : Hq * D].reshape(B, S, Hq, D), dq_f)
    _check("dw_q vs formula", wq.grad, dwq_f)


SHAPES = [(2, 67, 4, 2, 64), (2, 67, 4, 2, 128)]


@pytest.mark.parametrize("traditional", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_qk_norm_rope_fwd_bwd_matches_composition(ext, shape, traditional):
    _run_op_case(ext, *shape, traditional=traditional, offset=0)


@pytest.mark.parametrize("traditional", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_qk_norm_rope_forward_with_offset(ext, shape, traditional):
    from mlx_cuda_distributed_pretraining_amd.ops import qk_norm_rope
    from mlx_cuda_distributed_pretraining_amd.ops.rope import RopeTable

    B, S, Hq, Hkv, D = shape
    g = torch.Generator(device="cpu").manual_seed(32)
    qkv = _fused_qkv(g, B, S, Hq, Hkv, D)
    wq, wk = _weights(g, D)
    cos, sin = RopeTable(D, 10000.0).get(S, dev(), 5)
    q, k, _ = _views(qkv, Hq, Hkv, D)
    qo, ko = qk_norm_rope(q, k, wq, wk, cos, sin, EPS, traditional=traditional, offset=5)
    _check_fwd("q' offset=5", qo, _oracle(q.float(), wq.float(), cos, sin, traditional, 5))
    _check_fwd("k' offset=5", ko, _oracle(k.float(), wk.float(), cos, sin, traditional, 5))
    # offset really moves the rotation
    q0, _ = qk_norm_rope(q, k, wq, wk, cos, sin, EPS, traditional=traditional, offset=0)
    assert (q0.float() - qo.float()).abs().max().item() > 0.1


@pytest.mark.parametrize("shape", SHAPES)
def test_rstd_and_one_launch_weight_select(ext, shape):
    """The binding on the joint q|k view: rstd [B,S,H] fp32, and heads h < Hq
    take w_q, the rest w_k."""
    from mlx_cuda_distributed_pretraining_amd.ops.rope import RopeTable

    B, S, Hq, Hkv, D = shape
    g = torch.Generator(device="cpu").manual_seed(33)
    qkv = _fused_qkv(g, B, S, Hq, Hkv, D)
    wq, wk = _weights(g, D)
    cos, sin = RopeTable(D, 10000.0).get(S, dev(), 0)
    x = qkv[..., : (Hq + Hkv) * D].view(B, S, Hq + Hkv, D)
    y, rstd = ext.qknorm_rope_fwd(x, Hq, wq, wk, cos, sin, False, 0, EPS)
    assert y.shape == x.shape and rstd.shape == (B, S, Hq + Hkv) and rstd.dtype == torch.float32
    want = torch.rsqrt(x.float().pow(2).mean(-1) + EPS)
    rel = ((rstd - want).abs() / want).max().item()
    print(f"rstd: max rel err {rel:.3g}")
    assert rel < 1e-5
    _check_fwd("q heads", y[:, :, :Hq], _oracle(x[:, :, :Hq].float(), wq.float(), cos, sin, False, 0))
    _check_fwd("k heads", y[:, :, Hq:], _oracle(x[:, :, Hq:].float(), wk.float(), cos, sin, False, 0))


def test_more_rows_than_the_grid_cap(ext):
    """(1,4096,48 heads,64): 786432 lane groups against the 2048x256-thread
    grid cap, so the grid-stride loop takes a second trip (forward and
    backward, dw accumulated across trips)."""
    _run_op_case(ext, 1, 4096, 32, 16, 64, traditional=False, offset=0, seed=34,
                 on_device_rng=True)


@pytest.mark.parametrize("shape", [(2, 67, 4, 2, 128), (1, 4096, 32, 16, 64)])
def test_dw_is_deterministic(ext, shape):
    from mlx_cuda_distributed_pretraining_amd.ops.rope import RopeTable

    B, S, Hq, Hkv, D = shape
    gd = torch.Generator(device=dev()).manual_seed(35)
    qkv = torch.randn(B, S, (Hq + 2 * Hkv) * D, generator=gd, device=dev(),
                      dtype=torch.bfloat16)
    g_r = torch.randn(B, S, Hq + Hkv, D, generator=gd, device=dev(), dtype=torch.bfloat16)
    wq, wk = _weights(torch.Generator(device="cpu").manual_seed(35), D)
    cos, sin = RopeTable(D, 10000.0).get(S, dev(), 0)
    x = qkv[..., : (Hq + Hkv) * D].view(B, S, Hq + Hkv, D)
    _, rstd = ext.qknorm_rope_fwd(x, Hq, wq, wk, cos, sin, False, 0, EPS)
    outs = []
    for _ in range(2):
        dx = torch.empty(B, S, Hq + Hkv, D, device=dev(), dtype=torch.bfloat16)
        dw = ext.qknorm_rope_bwd(g_r, x, rstd, Hq, wq, wk, cos, sin, False, 0, dx)
        outs.append((dw, dx))
    assert outs[0][0].shape == (2, D) and outs[0][0].dtype == torch.float32
    assert torch.equal(outs[0][0], outs[1][0])
    assert torch.equal(outs[0][1], outs[1][1])


@pytest.mark.parametrize("traditional", [False, True])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("p", [0, 37])
def test_decode_kernel_bit_identical_to_forward(ext, p, D, traditional):
    from mlx_cuda_distributed_pretraining_amd.ops.rope import RopeTable

    B, Hq, Hkv = 3, 4, 2
    g = torch.Generator(device="cpu").manual_seed(36)
    qkv = _fused_qkv(g, B, 1, Hq, Hkv, D)
    wq, wk = _weights(g, D)
    cos, sin = RopeTable(D, 10000.0).get(64, dev(), 0)
    pos = torch.tensor([p], dtype=torch.int32, device=dev())
    x = qkv[..., : (Hq + Hkv) * D].view(B, 1, Hq + Hkv, D)  # batch-strided
    x0 = x.clone()
    y, _ = ext.qknorm_rope_fwd(x, Hq, wq, wk, cos, sin, traditional, p, EPS)
    v_before = qkv[..., (Hq + Hkv) * D :].clone()
    ext.qknorm_rope_decode_(x, Hq, wq, wk, cos, sin, traditional, pos, EPS)
    assert torch.equal(x, y)
    assert torch.equal(qkv[..., (Hq + Hkv) * D :], v_before)  # v slice untouched
    _check_fwd("decode q heads", x[:, :, :Hq],
               _oracle(x0[:, :, :Hq].float(), wq.float(), cos, sin, traditional, p))
    _check_fwd("decode k heads", x[:, :, Hq:],
               _oracle(x0[:, :, Hq:].float(), wk.float(), cos, sin, traditional, p))


def _doc_start(rows, S):
    out = torch.zeros(len(rows), S, dtype=torch.int32)
    for b, bounds in enumerate(rows):
        for lo in bounds:
            out[b, lo:] = lo
    return out.to(dev())


@pytest.mark.parametrize("doc_rows", [None, [[0, 37, 256], [0]]])
def test_fused_attention_node_matches_composition(ext, doc_rows):
    from mlx_cuda_distributed_pretraining_amd.ops import attention_ref
    from mlx_cuda_distributed_pretraining_amd.ops.attention import rope_flash_attention_qkv
    from mlx_cuda_distributed_pretraining_amd.ops.rope import RopeTable

    B, S, Hq, Hkv, D = 2, 300, 4, 2, 128
    g = torch.Generator(device="cpu").manual_seed(37)
    qkv = _fused_qkv(g, B, S, Hq, Hkv, D).requires_grad_(True)
    do = torch.randn(B, S, Hq, D, generator=g).to(dev(), torch.bfloat16)
    wq, wk = _weights(g, D)
    wq.requires_grad_(True)
    wk.requires_grad_(True)
    cos, sin = RopeTable(D, 10000.0).get(S, dev(), 0)
    doc_start = _doc_start(doc_rows, S) if doc_rows is not None else None

    o = rope_flash_attention_qkv(qkv, cos, sin, Hq, Hkv, D, causal=True, doc_start=doc_start,
                                 q_norm_weight=wq, k_norm_weight=wk, norm_eps=EPS)
    assert type(o.grad_fn).__name__ == "_QKNormRopeAttnQKVFnBackward"
    o.backward(do)

    qkv_f, wq_f, wk_f = _leaf(qkv), _leaf(wq), _leaf(wk)
    qf, kf, vf = _views(qkv_f, Hq, Hkv, D)
    o_ref = attention_ref(_oracle(qf, wq_f, cos, sin, False, 0),
                          _oracle(kf, wk_f, cos, sin, False, 0), vf, causal=True,
                          scale=1.0 / math.sqrt(D), doc_start=doc_start)
    o_ref.backward(do.float())

    _check_fwd("o", o, o_ref)
    _check("dqkv", qkv.grad, qkv_f.grad)
    _check("dw_q", wq.grad, wq_f.grad)
    _check("dw_k", wk.grad, wk_f.grad)


def test_without_weights_the_plain_node_runs(ext):
    from mlx_cuda_distributed_pretraining_amd.ops.attention import rope_flash_attention_qkv
    from mlx_cuda_distributed_pretraining_amd.ops.rope import RopeTable

    B, S, Hq, Hkv, D = 1, 64, 4, 2, 128
    qkv = _fused_qkv(torch.Generator(device="cpu").manual_seed(38), B, S, Hq, Hkv, D)
    qkv.requires_grad_(True)
    cos, sin = RopeTable(D, 10000.0).get(S, dev(), 0)
    o = rope_flash_attention_qkv(qkv, cos, sin, Hq, Hkv, D)
    assert type(o.grad_fn).__name__ == "_RopeAttnQKVFnBackward"
    with pytest.raises(ValueError):
        rope_flash_attention_qkv(qkv, cos, sin, Hq, Hkv, D, q_norm_weight=torch.ones(D))


def _model(qk_norm=True, **kw):
    from mlx_cuda_distributed_pretraining_amd.models.llama import Model, ModelArgs

    torch.manual_seed(0)
    args = ModelArgs(hidden_size=256, intermediate_size=512, num_layers=2,
                     num_heads=4, num_kv_heads=2, head_dim=128, vocab_size=503,
                     qk_norm=qk_norm, **kw)
    model = Model(args)
    _randomize_norms(model)
    return model.to(dev(), torch.bfloat16)


def test_model_matches_torch_path(ext, monkeypatch):
    """One bf16 forward + backward of a 2-layer qk_norm model on the HIP path
    vs the same weights with every op on its torch composition.

    The head is untied: with the tied head a random 2-layer model puts
    |logit| >= 4 on every token's own vocabulary row, where one bf16 ulp
    (2^-5 = 0.03125) is already above the 3e-2 forward bound, so two correct
    bf16 paths cannot be held to it (measured on an MI355X: exactly one ulp,
    0.03125, with qk_norm on and with it off). Untied, the logits stay below
    1 and the bound resolves several ulps."""
    model = _model(tie_word_embeddings=False).train()
    g = torch.Generator(device="cpu").manual_seed(39)
    x = torch.randint(0, 503, (2, 96), generator=g).to(dev())
    dy = torch.randn(2, 96, 503, generator=g).to(dev(), torch.bfloat16)

    def run():
        model.zero_grad(set_to_none=True)
        logits = model(x)
        logits.backward(dy)
        return logits.detach(), {n: p.grad.detach().clone() for n, p in model.named_parameters()}

    got_logits, got = run()
    monkeypatch.setenv("MCDP_FORCE_TORCH", "1")
    want_logits, want = run()
    monkeypatch.delenv("MCDP_FORCE_TORCH")

    _check_fwd("logits", got_logits, want_logits)
    for name in want:
        _check(name, got[name], want[name])
    for i in range(2):
        for n in ("q_norm", "k_norm"):
            assert want[f"layers.{i}.attention.{n}.weight"].abs().max().item() > 0


def test_graph_decode_matches_generate_step(ext):
    """GraphDecoder (eager-static and hipGraph-captured) vs generate_step with
    qk_norm=True, as test_static_decode_gpu_matches_eager does without it."""
    from mlx_cuda_distributed_pretraining_amd.inference.generate import generate_step
    from mlx_cuda_distributed_pretraining_amd.inference.static_decode import GraphDecoder

    model = _model().eval()
    prompt = [3, 17, 41, 5, 88, 23, 9, 101, 250, 77]
    n = 16
    oracle = list(generate_step(model, prompt, max_tokens=n))

    d1 = GraphDecoder(model, batch=1, max_len=512)
    d1.prefill(torch.tensor([prompt], device=dev()))
    got_eager = d1.decode(n)[0].tolist()
    assert got_eager == oracle, (got_eager, oracle)

    d2 = GraphDecoder(model, batch=1, max_len=512)
    d2.prefill(torch.tensor([prompt], device=dev()))
    d2.capture()
    got_graph = d2.decode(n)[0].tolist()
    assert got_graph == oracle, (got_graph, oracle)


@pytest.mark.parametrize("kv_bits", [None, 8])
def test_static_attend_batch2_matches_eager_branch(ext, monkeypatch, kv_bits):
    """StaticLayerCache.attend at batch 2 (q|k batch-strided inside qkv, one
    qknorm_rope_decode_ launch for both rows) against its own eager branch on
    the same state; the appended k row against the fp32 composition."""
    from mlx_cuda_distributed_pretraining_amd.inference.static_decode import StaticDecodeState

    model = _model().eval()
    attn = model.layers[0].attention
    B, P, Hq, Hkv, D = 2, 37, 4, 2, 128
    g = torch.Generator(device="cpu").manual_seed(40)
    qkv = _fused_qkv(g, B, 1, Hq, Hkv, D)
    k_hist = torch.randn(B, P, Hkv, D, generator=g).to(dev(), torch.bfloat16)
    v_hist = torch.randn(B, P, Hkv, D, generator=g).to(dev(), torch.bfloat16)
    codes = torch.randint(0, 256, (2, B, P, Hkv, D), generator=g).to(dev(), torch.uint8)

    def run():
        st = StaticDecodeState(model, batch=B, max_len=64, kv_bits=kv_bits)
        if kv_bits is None:
            st.k[0][:, :P] = k_hist
            st.v[0][:, :P] = v_hist
        else:  # history values code * 0.01 - 1.28
            st.k[0][:, :P] = codes[0]
            st.v[0][:, :P] = codes[1]
            for sz in (st.ksz[0], st.vsz[0]):
                sz[:, :P, :, :, 0] = 0.01
                sz[:, :P, :, :, 1] = -1.28
        st.pos.fill_(P)
        with torch.no_grad():
            o = st.layers[0].attend(attn, qkv.clone())
        return o, st.k[0][:, P].clone(), st.v[0][:, P].clone()

    o, k_new, v_new = run()
    monkeypatch.setenv("MCDP_FORCE_TORCH", "1")
    o_ref, _, _ = run()
    monkeypatch.delenv("MCDP_FORCE_TORCH")
    _check_fwd("o", o, o_ref)
    if kv_bits is None:
        _, k_in, v_in = _views(qkv, Hq, Hkv, D)
        st = StaticDecodeState(model, batch=B, max_len=64)
        want = _oracle(k_in.float(), attn.k_norm.weight.float(), st.cos, st.sin, False, P)
        _check_fwd("appended k row", k_new, want[:, 0])
        assert torch.equal(v_new, v_in[:, 0])
