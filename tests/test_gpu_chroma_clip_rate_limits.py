"""pc_chroma_clip_rate_sse_jobs past T = 64 (progressivecodec_amd/chroma_clip_rate.py, libpc_chroma_clip_rate.so): tiles whose block
partials take the final's second and third trip, the largest tiles of either depth, a job whose tile is clipped to a few rows, and
the refusal of T = 2048 at 10 bits.  One or two jobs each; every comparison is exact equality of integers.  Offsets past 2^31 are the
shared headers' code, exercised by tests/test_gpu_clip_rate.py."""
import numpy as np
import pytest
import torch

from tests import chroma_clip_rate_contract as JC
from tests import chroma_contract as CC
from tests.test_gpu_chroma_clip_rate import CR, DEV, hostile, jobs_raw
from tests.test_gpu_chroma_tiles import on_device
from tests.test_gpu_rate import POISON64

pytestmark = pytest.mark.gpu


def random_planes(fmt, H, W, seed):
    """a frame of random codes, without a batch axis, on the device"""
    g = np.random.default_rng(seed)
    semi, n, sh, _, _ = CC.FORMATS[fmt]
    Hc, Wc = CC.chroma_size(H, W, fmt)
    shapes = [(H, W), (Hc, Wc, 2)] if semi else [(H, W), (Hc, Wc), (Hc, Wc)]
    dt = np.uint16 if n == 10 else np.uint8
    return tuple(torch.from_numpy((g.integers(0, 2 ** n, s) << sh).astype(dt)).to(DEV) for s in shapes)


@pytest.mark.parametrize("fmt,siting,blocks", [("nv16", "left", 162), ("i444", "centre", 162), ("nv12", "topleft", 81)])
def test_tiles_of_576_take_the_finals_later_trips(fmt, siting, blocks):
    """T = 576: 162 block partials per job at sy = 1 (the final's lanes take l, l + 64 and l + 128: three trips), 81 at sy = 2 (two)"""
    cr = CR()
    from progressivecodec_amd import chroma_rate
    size, H, W, O = 576, 600, 1100, 32
    assert size * size // (2048 * CC.sub(fmt)[1]) == blocks
    g = cr.grid_of(H, W, size, O)
    assert (g.ny, g.nx) == (2, 2)
    fr = [CC.random_frame(1, H, W, fmt, seed=s, garbage=True) for s in (1, 2)]
    jobs = [(1, 0), (0, 3)]                                                # a full tile and the ragged corner
    x_np = hostile(2, seed=3, size=size)
    want = JC.job_sse(x_np, fr, jobs, H, W, size, O, fmt, "bt709", "limited", siting)
    x = torch.from_numpy(x_np).to(DEV)
    planes = [on_device(f) for f in fr]
    assert cr.tile_distortion_jobs(x, g, planes, jobs, fmt, siting=siting).tolist() == want
    odd = torch.zeros(x.numel() + 1, dtype=torch.float32, device=DEV)[1:].view(x.shape)
    odd.copy_(x)
    assert not cr.plan(odd, [[p[None] for p in ps] for ps in planes], fmt, overlap=O)
    assert cr.tile_distortion_jobs(odd, g, planes, jobs, fmt, siting=siting).tolist() == want
    for m, (f, t) in enumerate(jobs):
        assert chroma_rate.frame_tile_distortion(x[m:m + 1], g, planes[f], fmt, siting=siting, first_tile=t).tolist() == [want[m]]


@pytest.mark.parametrize("fmt,siting,size", [("nv12", "topleft", 2048), ("p210", "left", 1024)])
def test_the_largest_tiles_and_a_job_clipped_to_a_few_rows(fmt, siting, size):
    """the largest tile of the depth, one whole and one of which 5 rows and 40 columns lie inside the frame, against the frame call"""
    cr = CR()
    from progressivecodec_amd import chroma_rate
    H, W = size + 5, size + 40
    g = cr.grid_of(H, W, size, 0)
    assert (g.ny, g.nx) == (2, 2) and size == cr.max_tile(fmt)
    planes = [random_planes(fmt, H, W, seed=s) for s in (5, 6)]
    gen = torch.Generator(device=DEV).manual_seed(7)
    x = torch.rand((2, 3, size, size), generator=gen, device=DEV) * 1.5 - 0.25
    jobs = [(1, 0), (0, 3)]
    got = cr.tile_distortion_jobs(x, g, planes, jobs, fmt, siting=siting)
    for m, (f, t) in enumerate(jobs):
        one = chroma_rate.frame_tile_distortion(x[m:m + 1], g, planes[f], fmt, siting=siting, first_tile=t)
        assert torch.equal(got[m:m + 1], one) and all(v > 0 for v in one[0].tolist()), (m, f, t)
    assert got[0, 0].item() > got[1, 0].item() * 1000                      # 5 x 40 samples against 2048 x 2048


def test_a_tile_of_2048_at_10_bits_is_refused():
    cr = CR()
    H = W = 2100
    size = 2048
    planes = [random_planes("p210", H, W, seed=1)]
    x = torch.zeros((1, 3, size, size), dtype=torch.float32, device=DEV)
    with pytest.raises(ValueError, match="at most 1024"):
        cr.tile_distortion_jobs(x, cr.grid_of(H, W, size, 0), planes, [(0, 0)], "p210", siting="left")
    with pytest.raises(ValueError, match="at most 1024"):
        cr.encode_clip_to_size(None, planes, [0], 10 ** 9, "p210", siting="left", tile=size)
    table = [[p[None] for p in planes[0]]]
    rc, buf, ws_ok = jobs_raw(x, H, W, 0, "p210", "limited", "bt709", "left", table, [(0, 0)], size)
    torch.cuda.synchronize()
    assert rc == -1 and (buf == POISON64).all() and ws_ok
    rc, buf, ws_ok = jobs_raw(x, H, W, 0, "nv16", "limited", "bt709", "left", [[p[None] for p in random_planes("nv16", H, W, seed=2)]], [(0, 0)], size)
    assert rc == 0 and ws_ok and (buf[1] != POISON64).all() and np.all(buf[[0, 2]].cpu().numpy() == POISON64)
