"""GPU, two gloo ranks sharing the one MI355X of the test box (as tests/test_dist_gpu.py): fused gradient clipping under mvlt_amd.dist.DataParallel +
FusedAdamW + BF16Scaler(clip_grad=...).  G holds the rank SUM when the norm kernel runs and the 1/world is still owed: the norm must be that of the
MEAN gradient, the same on both ranks, and the clipped step must leave both ranks with the same moments and parameters."""
import hashlib
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
LT = dict(mlm=1, itm=1, t2i=1, cls=0)
T, IMG, B = 32, 64, 2
MAX_NORM = 1e-2                # far below the gradient norm of these batches (O(1)): the clip bites


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _model(seed=9):
    from mvlt_amd import pvlt
    from oracle import pvlt_oracle as O
    cfg = O.Cfg("pvlt_tiny", LT, 224, 768, T, 0.0)
    m = pvlt.pvlt_tiny(pretrained=False, token_hidden_size=768, num_text_tokens=T, loss_type=LT, pretrained_pth=None, drop_path_rate=0.0,
                       compute_dtype=torch.float32)
    m.load_state_dict(O.filled_state_dict(cfg, seed), strict=True)
    m.cuda()
    m.train()
    m.injected_masks = dict(bert=torch.ones(B, T, 768), droppath=[torch.ones(B)] * 8, droppath2=[torch.ones(B)] * 8)
    return m


def _batch(rank):
    from oracle import filler
    from oracle import pvlt_oracle as O
    b = O.to_torch_batch(filler.make_batch(70 + rank, B, IMG, T))
    if rank == 1:                       # unequal masked-token counts per rank, as in tests/test_dist_gpu.py
        b["mlm_labels"][0, 3] = b["ori_input_ids"][0, 3]
        b["mlm_labels"][1, 4] = b["ori_input_ids"][1, 4]
    return {k: v.cuda() for k, v in b.items()}


def _grads(model, batch, idx=1):
    from mvlt_amd.engine import train_step
    total, _ = train_step(model, batch, idx, True)
    for p in model.parameters():
        p.grad = None
    total.backward()
    torch.cuda.synchronize()
    return total


def _sha(t):
    return hashlib.sha256(t.detach().cpu().numpy().tobytes()).hexdigest()


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from mvlt_amd.dist import DataParallel
        from mvlt_amd.engine import BF16Scaler, train_step
        from mvlt_amd.optim import FusedAdamW
        core = _model(seed=9 + rank)                 # the wrapper broadcasts rank 0's weights
        model = DataParallel(core)
        opt = FusedAdamW(core, lr=1e-3, weight_decay=0.05)
        S = core.store
        total, _ = train_step(model, _batch(rank), 1, True)
        for p_ in model.parameters():
            p_.grad = None
        scaler = BF16Scaler()
        scaler(total, opt, clip_grad=MAX_NORM, parameters=model.parameters())
        torch.cuda.synchronize()
        assert S.pending_clip is None and S.pending_grad_scale == 1.0 and not S.scale_in_optimizer and not S.grad_works
        norm = float(scaler.last_grad_norm)
        # single-process reference, computed by every rank for itself (as tests/test_dist_gpu.py does): both batches through a plain model with rank 0's
        # weights, gradients averaged; the norm over the parameters' own elements in float64
        ref = _model(seed=9)
        gs = []
        for r in range(world):
            _grads(ref, _batch(r))
            gs.append(ref.store.G.clone())
        gmean = (sum(gs) / world).double()
        sq = sum(float((gmean[off:off + n] ** 2).sum()) for off, n, _ in ref.store.offsets.values())
        ref_norm = sq ** 0.5
        coef = min(1.0, MAX_NORM / (ref_norm + 1e-6))
        e_m = float((opt._m.double() - 0.1 * coef * gmean).norm() / (0.1 * coef * gmean).norm())
        q.put(dict(rank=rank, norm=norm, ref_norm=ref_norm, e_m=e_m, m_sha=_sha(opt._m), v_sha=_sha(opt._v), p_sha=_sha(S.P)))
    finally:
        dist.destroy_process_group()


def test_two_ranks_clip_the_mean_gradient(parity):
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted((q.get(timeout=600) for _ in range(world)), key=lambda d: d["rank"])
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    r0, r1 = res
    print(res)
    assert r0["norm"] == r1["norm"]
    assert r0["ref_norm"] > 10 * MAX_NORM                # the clip did bite
    for r in res:
        assert parity(f"dp-clip/norm-rank{r['rank']}", abs(r["norm"] - r["ref_norm"]) / r["ref_norm"], 1e-5), r
        # (the moments after one step from zero are (1 - beta1) * coef * mean gradient; the bound is tests/test_dist_gpu.py's on the gradients plus the norm's)
        assert parity(f"dp-clip/moment-rank{r['rank']}", r["e_m"], 2e-5), r
    assert r0["m_sha"] == r1["m_sha"] and r0["v_sha"] == r1["v_sha"]
    assert r0["p_sha"] == r1["p_sha"]
