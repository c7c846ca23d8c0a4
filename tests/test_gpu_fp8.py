"""The opt-in OCP e4m3 FeedForward path on the MI355X: the two kernels at the real shapes of the 640- / 1280-channel transformers (bounds derived
from the number formats, as in tests/test_linear_fp8.py), FeedForward.tokens_fp8 and the whole UNet against fake-quantised fp32 torch restatements
written here (the oracle sources stay untouched: its FeedForwards are wrapped on the instance), capture safety and the off switch.

Measured on an MI355X (fp16, [2,4,16,64,64], seeded weights; profiles/r07_fp8_parity.txt): see the docstring of
test_unet_fp8_against_the_fake_quantised_oracle."""
import os

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from animate_anything_amd import layers, ops
from util import FULL_UNET, SMALL_UNET, fullsize_inputs, fullsize_oracle, rel_err, seeded_state

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
FP8_MAX, TINY = 448.0, 1e-12


def dequant(q):
    return q.view(torch.float8_e4m3fn).float()


def fake_quant_rows(x):
    """The scale rule of aa_quant_rows_fp8 / ops.pack_weight_fp8 on the last dimension, in fp32: quantise to e4m3 (round to nearest even) and back."""
    s = x.abs().amax(dim=-1, keepdim=True).clamp_min(TINY) / FP8_MAX
    return (x / s).clamp(-FP8_MAX, FP8_MAX).to(torch.float8_e4m3fn).float() * s


def e4m3_step(v):
    return torch.exp2(torch.floor(torch.log2(v.abs().clamp_min(2.0 ** -6))) - 3)


# ------------------------------------------------------------------------------------------ the kernels at the real shapes
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("M,K,ln", [(34816, 640, True), (34816, 2560, False), (8704, 1280, True), (8704, 5120, False), (2176, 1280, True),
                                    (2176, 5120, False), (1027, 1280, True), (1027, 640, False)])
def test_quant_rows_real_shapes(M, K, dtype, ln):
    """The two uses of the model per level: LayerNorm inside at the transformer width, plain at the hidden width; 1027 rows: a ragged last workgroup.
    Bounds: tests/test_linear_fp8.py check_quant (half an e4m3 step at the element's magnitude + the stated fp32 rounding of the kernel)."""
    g = torch.Generator(device="cuda").manual_seed(M + K)
    x = (torch.randn(M, K, generator=g, device="cuda") * 2.0 + 0.3).to(dtype)
    x[M // 2] = 0
    if ln:
        gamma = (1.0 + 0.3 * torch.randn(K, generator=g, device="cuda")).to(dtype)
        beta = (0.2 * torch.randn(K, generator=g, device="cuda")).to(dtype)
        q, s = ops.quant_rows_fp8(x, ln=(gamma, beta, 1e-5))
        y = F.layer_norm(x.double(), (K,), gamma.double(), beta.double(), 1e-5).float()
    else:
        q, s = ops.quant_rows_fp8(x)
        y = x.float()
    torch.cuda.synchronize()
    assert not ((q & 0x7F) == 0x7F).any(), "NaN byte"
    amax = y.abs().amax(dim=1).clamp_min(TINY)
    want_s = (amax.double() / FP8_MAX)
    assert ((s.double() - want_s).abs() <= (2.0 ** -17 if ln else 2.0 ** -22) * want_s).all()
    sd = s.double()[:, None]
    err = (dequant(q).double() * sd - y.double()).abs()
    step = e4m3_step(y.double() / sd) * sd
    slack = y.abs().double() * (2.0 ** -18 if ln else 2.0 ** -21) + (amax.double()[:, None] * 2.0 ** -20 if ln else 0.0)
    print(f"quant_rows M={M} K={K} {dtype} ln={ln}: max err / (half step + slack) = {(err / (0.5 * step + slack)).max().item():.4f}")
    assert (err <= 0.5 * step + slack).all()


def unpack_rows(w, n):
    out = torch.empty_like(w)
    out[ops._fp8_row_perm(n, w.device)] = w
    return out


def linear_case(M, N, K, dtype, geglu, residual, seed=0):
    """As tests/test_linear_fp8.py linear_case, on the device and in row chunks (float64 products of the dequantised operands)."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, device="cuda")
    a = (r(M, K) * 2.0).half()
    w = (r(N, K) * K ** -0.5).half()
    b = (r(N) * 0.2).half()
    res = r(M, N // 2 if geglu else N).to(dtype) if residual else None
    pk = ops.pack_weight_fp8(w, b, geglu=geglu)
    q, s = ops.quant_rows_fp8(a)
    got = ops.linear_fp8(q, s, pk, residual=res, dtype=dtype)
    torch.cuda.synchronize()
    assert got.dtype == dtype and torch.isfinite(got.float()).all()
    wq = dequant(unpack_rows(pk.w, N)).double()
    sw = pk.scale.double()[None, :]
    worst, out_max = 0.0, got.float().abs().max().item()
    for m0 in range(0, M, 2048):
        sl = slice(m0, min(M, m0 + 2048))
        aq, sa = dequant(q[sl]).double(), s[sl].double()[:, None]
        y = (aq @ wq.T) * sa * sw + pk.bias.double()[None, :]
        acc_bound = K * 2.0 ** -24 * (aq.abs() @ wq.abs().T) * sa * sw
        rows = y.shape[0]
        if geglu:
            yb, ab = y.reshape(rows, N // 64, 2, 32), acc_bound.reshape(rows, N // 64, 2, 32)
            val, gate = yb[:, :, 0].reshape(rows, -1), yb[:, :, 1].reshape(rows, -1)
            want = val * F.gelu(gate)
            acc_bound = F.gelu(gate).abs() * ab[:, :, 0].reshape(rows, -1) + val.abs() * 1.13 * ab[:, :, 1].reshape(rows, -1)
        else:
            want = y if res is None else y + res[sl].double()
        ulp = torch.exp2(torch.floor(torch.log2(want.abs().clamp_min(2.0 ** -14))) - (10 if dtype == torch.float16 else 7))
        bound = 0.5 * ulp + acc_bound
        if geglu:                                              # tests/test_ff_fused.py: the fast-math erf-GELU against torch's
            bound = bound + 1e-2 * max(1.0, out_max)
        err = (got[sl].double() - want).abs()
        worst = max(worst, (err / bound).max().item())
    print(f"linear_fp8 M={M} N={N} K={K} {dtype} geglu={geglu} residual={residual}: max err / bound = {worst:.4f}")
    return worst


REAL = [(34816, 640), (8704, 1280), (2176, 1280)]            # (tokens, C) of the 32x32, 16x16 and 8x8 levels at [2,4,16,64,64]


@pytest.mark.parametrize("M,N,K", [(1, 640, 2560), (127, 1280, 5120), (129, 640, 2560), (300, 5120, 640)])
def test_linear_fp8_small_m(M, N, K):
    assert linear_case(M, N, K, torch.float16, False, True, seed=M) <= 1.0


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("M,C", REAL)
def test_linear_fp8_geglu_real_shapes(M, C, dtype):
    assert linear_case(M, 8 * C, C, dtype, True, False, seed=C) <= 1.0


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("M,C", REAL)
def test_linear_fp8_ff_out_real_shapes(M, C, dtype, residual):
    assert linear_case(M, C, 4 * C, dtype, False, residual, seed=C + 1) <= 1.0


def test_linear_fp8_exact_integers():
    """Exact integer data with an asymmetric weight matrix: the hardware's operand layout against the one the kernel (and the emulator) assume."""
    M, N, K = 130, 192, 256
    g = torch.Generator().manual_seed(9)
    a = torch.randint(-3, 4, (M, K), generator=g).float()
    w = torch.randint(-2, 3, (N, K), generator=g).float() + (torch.arange(N)[:, None] % 3 == 0).float()
    q = a.to(torch.float8_e4m3fn).view(torch.uint8).cuda()
    wq = w.to(torch.float8_e4m3fn).view(torch.uint8)
    pk = ops.PackedWeightFp8(wq[ops._fp8_row_perm(N, "cpu")].contiguous().cuda(), torch.ones(N).cuda(), None, N, K, False)
    got = ops.linear_fp8(q, torch.ones(M).cuda(), pk, dtype=torch.float16)
    assert torch.equal(got.float().cpu(), a @ w.T)


# ------------------------------------------------------------------------------------------ FeedForward.tokens_fp8
def fake_quant_ff(x, gamma, beta, eps, w1, b1, w2, b2, residual):
    """LayerNorm -> quantise / dequantise -> linear with fake-quantised weights -> erf-GEGLU -> quantise / dequantise -> linear -> + residual, fp32."""
    xn = x if gamma is None else F.layer_norm(x, (x.shape[-1],), gamma, beta, eps)
    y = F.linear(fake_quant_rows(xn), fake_quant_rows(w1), b1)
    val, gate = y.chunk(2, dim=-1)
    h = val * F.gelu(gate)
    return F.linear(fake_quant_rows(h), fake_quant_rows(w2), b2) + residual


@pytest.mark.parametrize("M,C", [(34816, 640), (8704, 1280), (2176, 1280), (333, 640)])
def test_feedforward_tokens_fp8(M, C):
    """Bound: that of the FeedForward tests (tests/test_ff_fused.py: max error <= 1e-2 max(1, range)).  The second quantisation sees an fp16-rounded
    activation in the product and an fp32 one here: elements on a rounding boundary land one e4m3 step apart - the share of output elements
    whose error exceeds a tenth of the bound is printed."""
    torch.manual_seed(C)
    ff = layers.FeedForward(C).eval()
    norm = layers.LayerNorm(C)
    with torch.no_grad():
        norm.weight.add_(0.3 * torch.randn(C))
        norm.bias.add_(0.2 * torch.randn(C))
    ff, norm = ff.half().cuda(), norm.half().cuda()
    g = torch.Generator(device="cuda").manual_seed(M)
    x = (torch.randn(M, C, generator=g, device="cuda") * 1.5 + 0.2).half()
    with torch.no_grad():
        got = ff.tokens_fp8(x, norm, residual=x).float()
        w1, w2 = ff.net[0].proj, ff.net[2]
        want = fake_quant_ff(x.float(), norm.weight.float(), norm.bias.float(), norm.eps, w1.weight.float(), w1.bias.float(),
                             w2.weight.float(), w2.bias.float(), x.float())
    err = (got - want).abs()
    scale = want.abs().max().item()
    bound = 1e-2 * max(1.0, scale)
    share = (err > 0.1 * bound).float().mean().item()
    print(f"tokens_fp8 M={M} C={C}: max err {err.max().item():.4g} (bound {bound:.4g}, range {scale:.4g}), share above a tenth of the bound {share:.3g}")
    assert torch.isfinite(got).all() and err.max().item() <= bound


# ------------------------------------------------------------------------------------------ the whole UNet
class FakeQuantFF(nn.Module):
    """Stands in for an oracle FeedForward (input = norm3's output): the arithmetic of FeedForward.tokens_fp8 in fp32, weights rounded to the product's
    storage type first (the product quantises its fp16 parameters)."""

    def __init__(self, ff, dtype):
        super().__init__()
        p1, p2 = ff.net[0].proj, ff.net[2]
        rt = lambda t: t.detach().to(dtype).float()
        for name, t in (("w1", fake_quant_rows(rt(p1.weight))), ("b1", rt(p1.bias)), ("w2", fake_quant_rows(rt(p2.weight))), ("b2", rt(p2.bias))):
            self.register_buffer(name, t)                     # (buffers: they follow the oracle to the device)

    def forward(self, x):
        val, gate = F.linear(fake_quant_rows(x), self.w1, self.b1).chunk(2, dim=-1)
        return F.linear(fake_quant_rows(val * F.gelu(gate)), self.w2, self.b2)


def wrap_oracle_feedforwards(ref, min_dim, dtype):
    import oracle
    n = 0
    for m in ref.modules():
        if isinstance(m, oracle.layers.BasicTransformerBlock) and m.ff.net[2].out_features >= min_dim:
            m.ff = FakeQuantFF(m.ff, dtype)
            n += 1
    return n


def test_unet_fp8_against_the_fake_quantised_oracle():
    """[2,4,16,64,64], fp16, switch on, hipGraph on, against the oracle with its >= 640-wide FeedForwards fake-quantised (same bound and form as
    tests/test_gpu_fullsize.py: latent MSE < 1e-3, max-normalised error < 3e-2); next to it the error against the PLAIN oracle golden, fp8 on and
    off (the number a user cares about).  The fake-quantised oracle runs in fp32 on the device.
    Measured on an MI355X (profiles/r07_fp8_parity.txt): on vs fake-quantised oracle MSE 8.71e-6 / max-normalised 0.0206;
    on vs plain oracle 2.095e-5 / 0.0359; off (fp16) vs plain oracle 1.542e-6 / 0.0086."""
    from animate_anything_amd.unet3d import UNet3DConditionModel
    DT = torch.float16
    plain = torch.load(os.path.join(HERE, "golden", "unet_fullsize_16x64x64.pt"))["out"].float()
    ref, state = fullsize_oracle()
    i = fullsize_inputs(16, 64)
    net = UNet3DConditionModel(**FULL_UNET).eval()
    net.load_state_dict(state)
    del state
    net = net.to(DT).cuda()
    net.enable_graph()
    dev = lambda x: x.to(DT).cuda()

    def product():
        with torch.no_grad():
            for _ in range(2):                                 # capture, then a replay
                out = net(dev(i["sample"]), i["t"], dev(i["text"]), dev(i["cond"]), dev(i["mask"]), motion=i["motion"]).sample
        torch.cuda.synchronize()
        return out.float().cpu()

    off = product()
    flagged = net.enable_fp8_feedforward()
    assert flagged > 0
    on = product()
    assert torch.isfinite(on).all() and not torch.equal(on, off)
    assert wrap_oracle_feedforwards(ref, 640, DT) == flagged
    ref = ref.cuda()
    f32 = lambda x: x.float().cuda()
    with torch.no_grad():
        want = ref(f32(i["sample"]), i["t"], f32(i["text"]), f32(i["cond"]), f32(i["mask"]), motion=i["motion"].cuda()).sample.float().cpu()
    mse_q, rel_q = ((on - want) ** 2).mean().item(), rel_err(on, want)
    mse_on, rel_on = ((on - plain) ** 2).mean().item(), rel_err(on, plain)
    mse_off, rel_off = ((off - plain) ** 2).mean().item(), rel_err(off, plain)
    print(f"fp8 on vs fake-quantised oracle: MSE {mse_q:.4g} max-normalised {rel_q:.4g}")
    print(f"fp8 on vs plain oracle:          MSE {mse_on:.4g} max-normalised {rel_on:.4g}")
    print(f"fp16   vs plain oracle:          MSE {mse_off:.4g} max-normalised {rel_off:.4g}")
    assert mse_q < 1e-3 and rel_q < 3e-2, (mse_q, rel_q)
    # Against the plain oracle the e4m3 path is NOT within twice the 16-bit figures (measured: MSE 2.095e-5 / max-normalised 0.0359 with the switch
    # on, 1.542e-6 / 0.0086 off: 13.6 x / 4.2 x), so the assertion is the measured value x 1.5 (the margin is for other noise realisations, as in
    # the 3-step parity test).  The max-normalised figure is above the 3e-2 the 16-bit path is held to: one reason the switch is off by default.
    assert mse_on <= 1.5 * 2.095e-5 and rel_on <= 1.5 * 0.0359, (mse_on, rel_on)
    assert mse_off < 1e-3 and rel_off < 3e-2, (mse_off, rel_off)


# ------------------------------------------------------------------------------------------ capture safety, the off switch
def _small_pipeline(fp8, graph):
    from animate_anything_amd.pipeline import LatentToVideoPipeline
    from animate_anything_amd.schedulers import DPMSolverMultistepScheduler
    from animate_anything_amd.unet3d import UNet3DConditionModel
    import oracle
    torch.manual_seed(0)
    state = seeded_state(oracle.UNet3DConditionModel(**SMALL_UNET).eval())
    unet = UNet3DConditionModel(**SMALL_UNET).eval()
    unet.load_state_dict(state)
    unet = unet.half().cuda()
    if fp8:
        assert unet.enable_fp8_feedforward(min_dim=128) > 0    # (the small architecture is 64 .. 256 wide; K must be a multiple of 128)
    unet.enable_graph(graph)
    return unet, LatentToVideoPipeline(vae=None, unet=unet, scheduler=DPMSolverMultistepScheduler())


def _three_steps(pipe):
    g = torch.Generator().manual_seed(4)
    r = lambda *s: torch.randn(*s, generator=g)
    frames, h, w = 3, 16, 16
    x0, pos, neg, init = r(1, 4, 1, h, w) * 0.5, r(1, 77, 128), r(1, 77, 128), r(1, 4, frames, h, w)
    mask = torch.zeros(1, 1, 1, h, w)
    mask[..., 4:12, 4:12] = 1
    dev = lambda t: t.half().cuda()
    _, lat = pipe(latents=init.cuda(), prompt_embeds=dev(pos), negative_prompt_embeds=dev(neg), condition_latent=dev(x0), mask=dev(mask),
                  motion=[4.0], num_inference_steps=3, guidance_scale=9.0, return_dict=False, output_type="latent")
    torch.cuda.synchronize()
    return lat.float().cpu()


def test_fp8_three_steps_captured_equal_eager():
    """Three pipeline steps with the switch on: hipGraph replay == eager launches, bit for bit (nothing in the branch depends on the host)."""
    _, pipe_g = _small_pipeline(True, True)
    _, pipe_e = _small_pipeline(True, False)
    a, b = _three_steps(pipe_g), _three_steps(pipe_e)
    assert torch.isfinite(a).all() and torch.equal(a, b)


def test_fp8_switch_off_leaves_no_state():
    """On, run, off: the output equals a never-switched model's bit for bit (and differs while the switch is on)."""
    unet, pipe = _small_pipeline(True, True)
    on = _three_steps(pipe)
    unet.disable_fp8_feedforward()
    off = _three_steps(pipe)
    _, fresh = _small_pipeline(False, True)
    never = _three_steps(fresh)
    assert torch.equal(off, never) and not torch.equal(on, never)
