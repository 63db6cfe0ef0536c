"""GPU parity of the U-Net forward and the integrators, through flocoder_amd.Unet -> C ABI -> HIP kernels.

Checked against (1) the golden vectors produced by the reference itself and (2) the CPU oracle on fresh seeded
inputs.  Tolerances (fp32 everywhere; differences are summation order + exp/erf ulps):
    single forward      rel-L2 <= 2e-5      trajectories (<= 64 forwards)   rel-L2 <= 2e-4
north_star's budget for decoded images is 1e-3."""
import os
import sys

import pytest
import torch

from conftest import ROOT, load_golden, rel_l2
from unet_taps import worst_sample
from oracle import flow_oracle as fo
from oracle.synth import synth_input, synth_state_dict

pytestmark = pytest.mark.gpu
FWD_TOL, TRAJ_TOL = 2e-5, 2e-4
DEV = "cuda:0"


def make_model(shapes, seed, **kw):
    from flocoder_amd.unet import Unet
    sd = synth_state_dict(shapes, seed)
    m = Unet(dim_mults=(1, 2, 4, 8), **kw).eval()
    missing, unexpected = m.load_state_dict(sd, strict=True), None
    return m.to(DEV), sd


def first_bad_tap(model, sd, x, t, cond, batch):
    """Localise a mismatch: compare every tapped block output with the oracle's."""
    from flocoder_amd._ops import fetch_tap
    taps = {}
    fo.unet_forward(sd, x, t, cond, taps=taps)
    rows = []
    for name, ref in taps.items():
        try:
            got = fetch_tap(model, name, batch).cpu()
        except ValueError:
            continue
        rows.append((name, rel_l2(got, ref)))
    return "\n".join(f"  {n:24s} {e:.3e}" for n, e in rows)


CASES = [("d32c102", 32, 1, 2, dict(dim=32, channels=4, n_classes=102)),
         ("d16c10", 16, 2, 3, dict(dim=16, channels=4, n_classes=10)),
         ("d8mask", 8, 3, 2, dict(dim=8, channels=4, n_classes=0, mask_cond=True))]


@pytest.mark.parametrize("tag,dim,seed,B,kw", CASES)
def test_forward_matches_reference_goldens(tag, dim, seed, B, kw):
    g = load_golden("g3_unet_" + tag)
    model, sd = make_model(g["shapes"], seed, **kw)
    x = synth_input("g3.x." + tag, (B, 4, dim, dim), seed)
    t = torch.from_numpy(g["t"])
    xd, td = x.to(DEV), t.to(DEV)

    def run(cond):
        c = None if cond is None else {k: (v.to(DEV) if v is not None else None) for k, v in cond.items()}
        with torch.no_grad():
            return model(xd, td, c).cpu()

    checks = []
    if "cls" in g:
        cls = torch.from_numpy(g["cls"])
        checks += [("v_class", {"class_cond": cls}), ("v_noclass", {"class_cond": None}), ("v_none", None)]
    if "mask" in g:
        mask = torch.from_numpy(g["mask"])
        checks += [("v_mask", {"class_cond": None, "mask_cond": mask}), ("v_ones", {"mask_cond": torch.ones_like(mask)}), ("v_none", None)]
    for key, cond in checks:
        out = run(cond)
        err = rel_l2(out, g[key])
        assert err < FWD_TOL, f"{tag}/{key}: rel-L2 {err:.3e}\n" + first_bad_tap(model, sd, x, t, cond, B)
    if tag == "d32c102":        # 1.0008 GFLOP per sample per NFE
        assert abs(model.flops_per_sample - 1.0008e9) / 1.0008e9 < 0.01, model.flops_per_sample


def test_forward_batch_sizes_and_determinism():
    """Odd batch sizes cross tile boundaries; repeated launches are bit-identical (no atomics anywhere)."""
    g = load_golden("g3_unet_d32c102")
    model, sd = make_model(g["shapes"], 1, dim=32, channels=4, n_classes=102)
    for B in (1, 5, 16):
        x = synth_input(f"bs.x{B}", (B, 4, 32, 32), 1)
        t = torch.linspace(1.0, 998.0, B)
        cls = torch.arange(B) % 102
        cls[0] = 101
        ref = fo.unet_forward(sd, x, t, {"class_cond": cls})
        with torch.no_grad():
            a = model(x.to(DEV), t.to(DEV), {"class_cond": cls.to(DEV)})
            b = model(x.to(DEV), t.to(DEV), {"class_cond": cls.to(DEV)})
        assert torch.equal(a, b)
        err = rel_l2(a.cpu(), ref)
        assert err < FWD_TOL, f"B={B}: {err:.3e}\n" + first_bad_tap(model, sd, x, t, {"class_cond": cls}, B)
        err = worst_sample(a, ref)                        # per sample: a batch-tail error is not diluted by the batch
        assert err < FWD_TOL, f"B={B}: worst sample {err:.3e}\n" + first_bad_tap(model, sd, x, t, {"class_cond": cls}, B)


@pytest.mark.parametrize("dim,H,W,B", [(32, 64, 64, 2), (16, 64, 64, 1), (32, 8, 8, 3), (32, 32, 16, 2), (64, 16, 16, 2)])
def test_forward_latent_sizes_vs_oracle(dim, H, W, B):
    """Other latent sizes put other attention kernels on the path: 64x64 latents run the bottleneck softmax attention and the
    8x8 linear attention with two 32-row tiles per head (linattn_sample.hip), 8x8 latents the n = 1 / 4 / 16 forms at C = 32..256,
    32x16 a non-square level, dim 64 the C = 512 levels (LDS-limit case of the per-head kernel)."""
    from flocoder_amd.unet import Unet
    torch.manual_seed(dim + H)
    m = Unet(dim=dim, dim_mults=(1, 2, 4, 8), channels=4, n_classes=10).eval()
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    g = torch.Generator().manual_seed(H * W + dim)
    for k, v in sd.items():                      # a fresh Unet has unit norms / zero biases: perturb so that every parameter matters
        if v.dtype == torch.float32 and v.ndim == 1:
            sd[k] = v + 0.1 * torch.randn(v.shape, generator=g)
    m.load_state_dict(sd, strict=True)
    m = m.to(DEV)
    x, t = torch.randn(B, 4, H, W, generator=g), torch.rand(B, generator=g) * 999
    cls = torch.arange(B) % 10
    ref = fo.unet_forward(sd, x, t, {"class_cond": cls})
    with torch.no_grad():
        out = m(x.to(DEV), t.to(DEV), {"class_cond": cls.to(DEV)})
    err = rel_l2(out.cpu(), ref)
    assert err < FWD_TOL, f"dim={dim} {H}x{W}: {err:.3e}\n" + first_bad_tap(m, sd, x, t, {"class_cond": cls}, B)


def test_rk4_and_euler_trajectories_match_reference_goldens():
    from flocoder_amd import sampling as S
    g = load_golden("g5_trajectories")
    model, sd = make_model(g["shapes"], 5, dim=16, channels=4, n_classes=10)
    src = synth_input("g5.src", (2, 4, 16, 16), 5).to(DEV)
    cls = torch.from_numpy(g["cls"]).to(DEV)
    for cfg in (0, 3):
        lat, nfe = S.generate_latents_rk4(model, (2, 4, 16, 16), n_steps=5, cond={"class_cond": cls}, cfg_strength=float(cfg), source=src.clone())
        assert nfe == 20
        assert rel_l2(lat.cpu(), g[f"rk4_n5_cfg{cfg}"]) < TRAJ_TOL, cfg
        assert worst_sample(lat, g[f"rk4_n5_cfg{cfg}"]) < TRAJ_TOL, cfg
    lat, _ = S.generate_latents_rk4(model, (2, 4, 16, 16), n_steps=4, cond={}, cfg_strength=3.0, source=src.clone())
    assert rel_l2(lat.cpu(), g["rk4_n4_nocond"]) < TRAJ_TOL
    assert worst_sample(lat, g["rk4_n4_nocond"]) < TRAJ_TOL
    init = synth_input("g5.init", (2, 4, 16, 16), 5).to(DEV)
    lat, nfe = S.generate_latents_rk4(model, (2, 4, 16, 16), n_steps=8, cond={"class_cond": cls}, cfg_strength=3.0, source=src.clone(),
                                      init_latents=init, init_strength=0.5)
    assert nfe == 16 and rel_l2(lat.cpu(), g["rk4_n8_init05"]) < TRAJ_TOL
    assert worst_sample(lat, g["rk4_n8_init05"]) < TRAJ_TOL
    for n in (4, 16):
        lat, nfe = S.euler_sampler(model, (2, 4, 16, 16), n, cond=cls, source=src)
        assert nfe == n and rel_l2(lat.cpu(), g[f"euler_n{n}"]) < TRAJ_TOL, n
        assert worst_sample(lat, g[f"euler_n{n}"]) < TRAJ_TOL, n
    # generate_latents dispatch + graph replay of a cached variant gives the same bits
    a, _ = S.generate_latents(model, (2, 4, 16, 16), "rk4", 5, {"class_cond": cls}, 3.0, source=src.clone())
    b, _ = S.generate_latents(model, (2, 4, 16, 16), "rk4", 5, {"class_cond": cls}, 3.0, source=src.clone())
    assert torch.equal(a, b) and rel_l2(a.cpu(), g["rk4_n5_cfg3"]) < TRAJ_TOL
    assert worst_sample(a, g["rk4_n5_cfg3"]) < TRAJ_TOL


def test_euler64_flowers_shape_vs_oracle():
    """BASELINE config 2 at reduced batch: 64-step Euler, 4x32x32, dim=32, n_classes=102, against the CPU oracle."""
    from flocoder_amd import sampling as S
    g = load_golden("g3_unet_d32c102")
    model, sd = make_model(g["shapes"], 1, dim=32, channels=4, n_classes=102)
    B = 3
    src = synth_input("e64.src", (B, 4, 32, 32), 1)
    cls = torch.tensor([5, 77, 101])
    ref, _ = fo.euler_sampler(sd, src, 64, cls)
    lat, nfe = S.euler_sampler(model, (B, 4, 32, 32), 64, cond=cls.to(DEV), source=src.to(DEV))
    assert nfe == 64
    err = rel_l2(lat.cpu(), ref)
    assert err < TRAJ_TOL, f"{err:.3e}"
    err = worst_sample(lat, ref)
    assert err < TRAJ_TOL, f"worst sample {err:.3e}"
    # linearity-free sanity property at a size the oracle would not finish quickly: batch independence
    big = synth_input("e64.big", (32, 4, 32, 32), 1).to(DEV)
    big[:B] = src.to(DEV)
    ids = torch.cat([cls, torch.arange(29) % 102]).to(DEV)
    lat2, _ = S.euler_sampler(model, (32, 4, 32, 32), 64, cond=ids, source=big)
    assert rel_l2(lat2[:B].cpu(), lat.cpu()) < 1e-5      # a sample's trajectory does not depend on its batch mates
    assert worst_sample(lat2[:B], lat) < 1e-5


def test_mask_cond_sampling_vs_oracle():
    from flocoder_amd import sampling as S
    g = load_golden("g3_unet_d8mask")
    model, sd = make_model(g["shapes"], 3, dim=8, channels=4, n_classes=0, mask_cond=True)
    src = synth_input("mk.src", (2, 4, 8, 8), 3)
    mask = torch.from_numpy(g["mask"])
    ref, _ = fo.generate_latents_rk4(sd, src.clone(), 6, {"class_cond": None, "mask_cond": mask}, 3.0)
    lat, _ = S.generate_latents_rk4(model, (2, 4, 8, 8), 6, {"class_cond": None, "mask_cond": mask.to(DEV)}, 3.0, source=src.to(DEV))
    assert rel_l2(lat.cpu(), ref) < TRAJ_TOL
    ones = torch.ones_like(mask)
    ref, _ = fo.generate_latents_rk4(sd, src.clone(), 4, {"mask_cond": ones}, 3.0)
    lat, _ = S.generate_latents_rk4(model, (2, 4, 8, 8), 4, {"mask_cond": ones.to(DEV)}, 3.0, source=src.to(DEV))
    assert rel_l2(lat.cpu(), ref) < TRAJ_TOL


def test_bench_batch_forward_with_fused_tails():
    """The fused Block tails (fc_debug_set_fused_tail(1): workgroups of a sample meet at a device counter and finish
    SiLU(GN(.)) + res from their accumulators) at B=64, the launch sizes bench.py runs: no timed-out wait, same results."""
    from flocoder_amd import _binding as B
    from flocoder_amd.unet import Unet
    B.check(B.lib().fc_debug_set_fused_tail(1))
    try:
        _fused_tail_body(Unet)
    finally:
        B.check(B.lib().fc_debug_set_fused_tail(-1))      # back to the default: later tests in this process build default plans


def _fused_tail_body(Unet):
    torch.manual_seed(0)
    m = Unet(dim=32, dim_mults=(1, 2, 4, 8), channels=4, n_classes=102).eval()
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    m = m.to(DEV)
    g = torch.Generator().manual_seed(4)
    x, t = torch.randn(64, 4, 32, 32, generator=g), torch.rand(64, generator=g) * 999
    ids = torch.randint(0, 102, (64,), generator=g)
    with torch.no_grad():
        v = m(x.to(DEV), t.to(DEV), {"class_cond": ids.to(DEV)})
        v2 = m(x.to(DEV), t.to(DEV), {"class_cond": ids.to(DEV)})
    assert m.fused_tail_errors() == 0
    assert torch.equal(v, v2)
    assert any("+fin" in r["kernel"] for r in m.profile_ops(64, repeats=1))          # the fused path is the one that ran
    ref = fo.unet_forward(sd, x[:8], t[:8], {"class_cond": ids[:8]})
    assert rel_l2(v[:8].cpu(), ref) < FWD_TOL
    assert worst_sample(v[:8], ref) < FWD_TOL
    assert m.fused_tail_errors() == 0


_FOLD_SCRIPT = r"""
import sys, torch
sys.path.insert(0, %r)
from flocoder_amd.unet import Unet
from flocoder_amd.codecs import SD_VAE_Wrapper
torch.manual_seed(31)
m = Unet(dim=32, dim_mults=(1, 2, 4, 8), channels=4, n_classes=102).eval().to("cuda:0")
g = torch.Generator().manual_seed(32)
x = torch.randn(6, 4, 32, 32, generator=g).to("cuda:0"); ids = torch.randint(102, (6,), generator=g).to("cuda:0")
t = torch.full((6,), 333.0, device="cuda:0")
with torch.no_grad():
    v = m(x, t, {"class_cond": ids}).clone()
executed = sum(r["flops_per_sample"] for r in m.profile_ops(6, repeats=1))
w = SD_VAE_Wrapper(weights="random", seed=7).eval().to("cuda:0")
z = (torch.randn(2, 4, 32, 32, generator=g) * 4.5).to("cuda:0")
img = w.decode(z)
torch.save((v.cpu(), img.cpu(), m.flops_per_sample, executed), sys.argv[1])
"""


def test_folded_upsampling_equals_the_conv_over_the_upsampled_window(tmp_path):
    """Upsample = nn.Upsample(scale_factor=2, nearest) + Conv2d(3x3, padding 1) (unet.py:42-46; AutoencoderKL's Upsample2D behind
    codecs.py:631-652).  Output pixel (2y + a, 2x + b) only ever sees a 2x2 block of source pixels, each through the sum of the taps that land
    on it, so inference plans run four 2x2 convolutions on the low-resolution tensor (plan.h conv_up2, PACK_UP4 / PACK_UP4_B3) -- 4/9 of the
    multiply-adds, exact in real arithmetic.  FLOCODER_AMD_UPS_FOLD=0 keeps the 3x3 form: same result to fp32 rounding for the U-Net's three
    Upsample layers and the SD-VAE decoder's three; the FLOPs per sample stay the reference's figure, the executed ones drop."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    outs = {}
    for tag, env in (("folded", {}), ("plain", {"FLOCODER_AMD_UPS_FOLD": "0"})):
        f = str(tmp_path / (tag + ".pt"))
        e = dict(os.environ); e.update(env)
        r = subprocess.run([sys.executable, "-c", _FOLD_SCRIPT % root, f], env=e, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        outs[tag] = torch.load(f)
    (v, img, fl, ex), (v0, img0, fl0, ex0) = outs["folded"], outs["plain"]
    print("folded vs 3x3 upsampling: U-Net forward rel-L2 %.2e, SD-VAE decode %.2e; GFLOP/sample reference %.4f executed %.4f (plain %.4f)"
          % (rel_l2(v, v0), rel_l2(img, img0), fl / 1e9, ex / 1e9, ex0 / 1e9))
    assert torch.isfinite(v).all() and torch.isfinite(img).all()
    # (either form is ~2e-6 from the fp64-accumulating oracle on this decoder: tests/test_gpu_vae.py)
    assert rel_l2(v, v0) < 2e-6 and rel_l2(img, img0) < 1e-5
    assert fl == fl0 and abs(ex0 - fl0) < 1e-3 * fl0 and ex < 0.95 * ex0


@pytest.mark.parametrize("H,W,kw,need_kernel", [(8, 16, dict(n_classes=10), True), (16, 8, dict(n_classes=0, mask_cond=True), None), (8, 8, dict(n_classes=10), True)])
def test_one_workgroup_per_sample_kernel_other_shapes_vs_oracle(H, W, kw, need_kernel):
    """The steps of csrc/unet_sample.hip that the square 8x8 golden model does not reach: non-square latents put TWO positions on the
    bottleneck (the general full-attention step instead of the one-position closed form), 8x16 a linear attention over 128 positions (the
    general sequential-heads step), class conditioning the FiLM rows of the embedding table; the mask-conditioned 16x8 model does not fit a
    CU's LDS and must come out right on the ordinary plan it falls back to.
    Against the CPU oracle, with perturbed norm parameters so that every parameter matters."""
    from flocoder_amd.unet import Unet
    torch.manual_seed(H * 31 + W)
    m = Unet(dim=8, dim_mults=(1, 2, 4, 8), channels=4, **kw).eval()
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    g = torch.Generator().manual_seed(H * W + 8)
    for k, v in sd.items():
        if v.dtype == torch.float32 and v.ndim == 1:
            sd[k] = v + 0.1 * torch.randn(v.shape, generator=g)
    m.load_state_dict(sd, strict=True)
    m = m.to(DEV)
    Bn = 5
    x, t = torch.randn(Bn, 4, H, W, generator=g), torch.rand(Bn, generator=g) * 999
    if kw.get("mask_cond"):
        cond = {"mask_cond": (torch.rand(Bn, 4, H, W, generator=g) > 0.4).float()}
    else:
        cls = torch.arange(Bn) % 10
        cls[0] = 9
        cond = {"class_cond": cls}
    ref = fo.unet_forward(sd, x, t, cond)
    with torch.no_grad():
        out = m(x.to(DEV), t.to(DEV), {k: v.to(DEV) for k, v in cond.items()})
    print(f"{H}x{W} {kw}: {m.launches_per_forward} launches per forward")
    if need_kernel:
        assert m.launches_per_forward <= 4, m.launches_per_forward          # conditioning + the ONE U-Net launch
    err = rel_l2(out.cpu(), ref)
    assert err < FWD_TOL, f"{H}x{W} {kw}: {err:.3e} with {m.launches_per_forward} launches"


def test_one_workgroup_per_sample_kernel_samplers_vs_oracle():
    """The integrators on the per-sample kernel: legacy Euler (the kernel's own Euler tail: y += v dt, the counters moved by the workgroup that
    finishes last) and RK4 with classifier-free guidance (2B rows per evaluation, conditioning rows from the precomputed table), a
    class-conditioned dim-8 model at 8x8 against the CPU oracle; replays of the cached graph give the same bits."""
    from flocoder_amd import sampling as S
    from flocoder_amd.unet import Unet
    torch.manual_seed(77)
    m = Unet(dim=8, dim_mults=(1, 2, 4, 8), channels=4, n_classes=10).eval()
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    g = torch.Generator().manual_seed(78)
    for k, v in sd.items():
        if v.dtype == torch.float32 and v.ndim == 1:
            sd[k] = v + 0.1 * torch.randn(v.shape, generator=g)
    m.load_state_dict(sd, strict=True)
    m = m.to(DEV)
    Bn = 6
    src = torch.randn(Bn, 4, 8, 8, generator=g)
    cls = torch.tensor([0, 3, 9, 9, 5, 1])
    ref, _ = fo.euler_sampler(sd, src, 12, cls)
    lat, nfe = S.euler_sampler(m, (Bn, 4, 8, 8), 12, cond=cls.to(DEV), source=src.to(DEV))
    assert nfe == 12 and m.launches_per_forward <= 4
    assert rel_l2(lat.cpu(), ref) < TRAJ_TOL
    again, _ = S.euler_sampler(m, (Bn, 4, 8, 8), 12, cond=cls.to(DEV), source=src.to(DEV))
    assert torch.equal(again, lat)
    ref, _ = fo.generate_latents_rk4(sd, src.clone(), 7, {"class_cond": cls}, 3.0)
    lat, nfe = S.generate_latents_rk4(m, (Bn, 4, 8, 8), 7, {"class_cond": cls.to(DEV)}, 3.0, source=src.to(DEV))
    assert nfe == 28 and rel_l2(lat.cpu(), ref) < TRAJ_TOL
    again, _ = S.generate_latents_rk4(m, (Bn, 4, 8, 8), 7, {"class_cond": cls.to(DEV)}, 3.0, source=src.to(DEV))
    assert torch.equal(again, lat)


def test_one_workgroup_per_sample_kernel_is_the_default_where_it_fits_and_both_plans_match_the_goldens():
    """csrc/unet_sample.hip (the whole forward of a sample in one workgroup, for models whose activations fit a CU's LDS and batches of at
    most one sample per CU): the mask-conditioned dim-8 model runs on it by default (the plan is ONE U-Net launch),
    a batch larger than the CU count keeps the ordinary plan, and with FLOCODER_AMD_SAMPLE_KERNEL=0 the ordinary plan gives the goldens,
    the mask-conditioned sampler and the oracle the same answers (a child process: the switch is read once per process)."""
    import subprocess
    g = load_golden("g3_unet_d8mask")
    model, _ = make_model(g["shapes"], 3, dim=8, channels=4, n_classes=0, mask_cond=True)
    x = synth_input("g3.x.d8mask", (2, 4, 8, 8), 3).to(DEV)
    t = torch.from_numpy(g["t"]).to(DEV)
    with torch.no_grad():
        small = model(x, t, None)
        n_small = model.launches_per_forward
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        reps = cus // 2 + 1                                                   # 2 * reps samples > the CU count
        big = model(x.repeat(reps, 1, 1, 1), t.repeat(reps), None)
        n_big = model.launches_per_forward
    assert n_small <= 4 < n_big, (n_small, n_big)                             # conditioning + ONE U-Net launch, against the ~115 of the ordinary plan
    assert rel_l2(big[:2].cpu(), small.cpu()) < 2e-6                          # the two plans agree (summation order apart)
    assert worst_sample(big, small.repeat(reps, 1, 1, 1)) < 2e-6              # every row of the ordinary plan's batch, tail included
    env = dict(os.environ, FLOCODER_AMD_SAMPLE_KERNEL="0")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-q", "-x", "-p", "no:cacheprovider",
                        "-k", "d8mask or mask_cond_sampling"], env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    tail = r.stdout.strip().splitlines()[-1] if r.stdout.strip() else ""
    assert r.returncode == 0 and " passed" in tail and "no tests ran" not in tail, (r.returncode, r.stdout[-2000:], r.stderr[-500:])
