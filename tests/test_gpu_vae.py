"""GPU parity of the SD-VAE codec (through the C ABI) against oracle/sdvae_oracle.py on seeded random weights.
PARITY UNPINNED for this codec: diffusers + weights are absent, so this is GPU<->CPU self-consistency of the restated
architecture.  Tolerance rel-L2 <= 2e-4 over ~30 stacked fp32 convolutions."""
import pytest
import torch

from conftest import rel_l2
from oracle import sdvae_oracle as vo

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 2e-4


@pytest.fixture(scope="module")
def codec():
    from flocoder_amd.codecs import SD_VAE_Wrapper
    w = SD_VAE_Wrapper(weights="random", seed=7).eval().to(DEV)
    sd = {k[4:]: v.detach().cpu() for k, v in w.state_dict().items()}
    return w, sd


def test_encode_mean_matches_oracle(codec):
    w, sd = codec
    g = torch.Generator().manual_seed(11)
    x = torch.rand(2, 3, 64, 64, generator=g) * 2 - 1
    ref = vo.encode_mean(sd, x)
    z = w.encode(x.to(DEV))
    assert z.shape == (2, 4, 8, 8)
    assert rel_l2(z.cpu(), ref) < TOL


def test_decode_matches_oracle_and_batch_independence(codec):
    w, sd = codec
    g = torch.Generator().manual_seed(12)
    z = torch.randn(3, 4, 8, 8, generator=g) * 4.5          # unscaled SD latents
    ref = vo.decode(sd, z)
    y = w.decode(z.to(DEV))
    assert y.shape == (3, 3, 64, 64)
    assert rel_l2(y.cpu(), ref) < TOL
    y1 = w.decode(z[1:2].to(DEV))                            # a sample decodes the same alone as inside a batch
    assert rel_l2(y1.cpu(), y[1:2].cpu()) < 1e-5
    assert torch.equal(w.decode(z.to(DEV)), y)               # and launches are bit-reproducible


def test_forward_roundtrip_protocol(codec):
    w, sd = codec
    x = torch.rand(1, 3, 64, 64, generator=torch.Generator().manual_seed(13))
    recon, loss, stats = w(x.to(DEV), get_stats=True)
    assert recon.shape == x.shape and loss == 0.0 and "codebook_mean_dist" in stats
    assert rel_l2(recon.cpu(), vo.decode(sd, vo.encode_mean(sd, x))) < 2 * TOL
    # decode analytic work per sample scales with pixels: 622.2 GFLOP at 256^2 -> /16 at 64^2
    assert abs(w.flops_per_sample(decode=True) - 622.2e9 / 16) / (622.2e9 / 16) < 0.02


def test_sampler_decodes_on_device(codec):
    """sampler() end to end: U-Net integration + codec.decode, chunked on the device (sampling.py:186-229)."""
    from flocoder_amd.sampling import sampler
    from flocoder_amd.unet import Unet
    w, sd = codec
    torch.manual_seed(0)
    model = Unet(dim=8, channels=4, n_classes=3).eval().to(DEV)
    lat, img, nfe = sampler(model, w, method="rk4", batch_size=4, n_steps=3, cond={"class_cond": torch.tensor([0, 1, 2, 1], device=DEV)},
                            latent_shape=(4, 8, 8), cfg_strength=2.0)
    assert lat.shape == (4, 4, 8, 8) and img.shape == (4, 3, 64, 64) and nfe == 12 and torch.isfinite(img).all()


def test_split_bf16_decode_is_within_the_image_gate_and_opt_in():
    """Opt-in split-bf16 arithmetic of the codec (fc_vae_set_precision; secondary numbers only, never the headline): the decoded 256x256 images
    against the exact-fp32 decode of the same latents and against the oracle -- within 1e-3 rel-L2 with a wide margin (measured ~1e-5),
    different bits from the fp32 decode, and switching back restores the exact result."""
    from flocoder_amd.codecs import SD_VAE_Wrapper
    w = SD_VAE_Wrapper(weights="random", seed=7).eval().to(DEV)
    sd = {k[4:]: v.detach().cpu() for k, v in w.state_dict().items()}
    g = torch.Generator().manual_seed(14)
    z = torch.randn(2, 4, 32, 32, generator=g) * 4.5
    exact = w.decode(z.to(DEV))
    w.set_precision("bf16x3")
    fast = w.decode(z.to(DEV))
    e = rel_l2(fast, exact)
    eo = rel_l2(fast[:1].cpu(), vo.decode(sd, z[:1]))
    print("SD-VAE decode 256x256, split-bf16 vs fp32: rel-L2 %.2e; vs oracle %.2e" % (e, eo))
    assert torch.isfinite(fast).all() and 0.0 < e < 2e-4 and eo < 1e-3
    ze = w.encode(exact)                                        # the encoder follows the same switch
    w.set_precision("fp32")
    assert torch.equal(w.decode(z.to(DEV)), exact)
    assert rel_l2(ze, w.encode(exact)) < 2e-4
    with pytest.raises(ValueError):
        w.set_precision("fp16")
