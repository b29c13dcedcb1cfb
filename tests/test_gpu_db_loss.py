"""GPU parity of the fused DreamBooth PSO loss kernels (csrc/db_loss.hip) against the oracle restatement of
DB:1847-1935 (oracle/pso_math.py; parity unpinned beyond that restatement -- the DreamBooth trainer cannot be
imported here and ships no golden vectors)."""
import numpy as np
import pytest
import torch

from oracle import pso_math

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("loss_type", ["pso", "pso_db"])
# the first three keep their ids from when the shape was (2B, 4, h, h): B-h-eps_bf16, seed 100 B + h
@pytest.mark.parametrize("B,n,seed,eps_bf16", [
    pytest.param(1, 4 * 64 * 64, 164, True, id="1-64-True"), pytest.param(2, 4 * 32 * 32, 232, False, id="2-32-False"),
    pytest.param(3, 4 * 16 * 16, 316, True, id="3-16-True"),
    (1, 8196, 1, True), (1, 8196, 1, False),        # second chunk of 4 elements (DB_CHUNK = 8192)
    (2, 17412, 2, True), (2, 17412, 2, False),      # three chunks, the last ragged against the thread stride
    (300, 4, 3, True), (300, 4, 3, False),          # the finalize loops over pairs take a second trip
    (1024, 4, 4, True), (1024, 4, 4, False)])       # ... and fill the 1024-entry LDS tables
def test_db_loss_fwd_bwd_vs_oracle(cuda, loss_type, B, n, seed, eps_bf16):
    from pairwise_sample_optimization_amd import kernels as K
    rng = np.random.default_rng(seed)
    shape = (2 * B, n)
    sig = rng.choice([14.614647, 4.081731, 1.612887, 0.693205], size=B).astype(np.float32)
    sigma = np.concatenate([sig, sig])
    x0 = rng.standard_normal(shape).astype(np.float32)
    noise = rng.standard_normal(shape).astype(np.float32)
    noisy = (x0 + noise * sigma[:, None]).astype(np.float32)
    eps = (noise + 0.05 * rng.standard_normal(shape)).astype(np.float32)
    eps_ref = (noise + 0.05 * rng.standard_normal(shape)).astype(np.float32)
    if eps_bf16:  # the kernel reads the UNet's bf16 output; give the oracle the same rounded values
        eps = torch.from_numpy(eps).bfloat16().float().numpy()
        eps_ref = torch.from_numpy(eps_ref).bfloat16().float().numpy()
    beta, nd, pw = (5.0, 0.1, 0.5) if loss_type == "pso_db" else (20.0, 0.1, 1.0)
    lt = K.DB_HINGE if loss_type == "pso_db" else K.DB_SIGMOID
    dt = torch.bfloat16 if eps_bf16 else torch.float32
    e = torch.from_numpy(eps).to(cuda, dt)
    er = torch.from_numpy(eps_ref).to(cuda, dt) if loss_type == "pso" else None
    nz, t, s = (torch.from_numpy(a).to(cuda) for a in (noisy, x0, sigma))
    ws = K.db_loss_ws(B, eps[0].size, cuda)
    loss, losses, logits = K.db_loss_fwd(lt, e, nz, t, s, beta, nd, pw, ws, eps_ref=er)
    deps = K.db_loss_bwd(lt, e, nz, t, s, beta, nd, pw, ws, grad_scale=0.5, out_dtype=torch.float32)
    rloss, rl, rlog = pso_math.db_loss(eps, noisy, x0, sigma, beta, nd, pw, loss_type, eps_ref)
    rg = 0.5 * pso_math.db_loss_deps(eps, noisy, x0, sigma, beta, nd, pw, loss_type, eps_ref)
    np.testing.assert_allclose(losses[:2 * B].cpu().numpy(), rl, rtol=2e-6)
    np.testing.assert_allclose(logits.cpu().numpy(), rlog, rtol=1e-4, atol=1e-6)
    assert abs(loss.item() - rloss) <= 2e-5 * abs(rloss) + 1e-7
    g = deps.cpu().numpy()
    assert np.abs(g - rg).max() <= 1e-4 * np.abs(rg).max() + 1e-12


def test_db_loss_rejects_more_than_1024_pairs(cuda):
    from pairwise_sample_optimization_amd import kernels as K, _lib
    B = 1025
    e = torch.zeros((2 * B, 4), device=cuda)
    s = torch.ones(2 * B, device=cuda)
    ws = K.db_loss_ws(B, 4, cuda)
    with pytest.raises(_lib.PsoLibError):
        K.db_loss_fwd(K.DB_HINGE, e, e, e, s, 5.0, 0.1, 0.5, ws)
    with pytest.raises(_lib.PsoLibError):
        K.db_loss_bwd(K.DB_HINGE, e, e, e, s, 5.0, 0.1, 0.5, ws)
