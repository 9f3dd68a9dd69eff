"""GPU, two gloo ranks sharing the one MI355X of the test box (as tests/test_clip_dist_gpu.py): the non-finite-gradient guard under
mvlt_amd.dist.DataParallel + FusedAdamW(skip_nonfinite=True) + BF16Scaler(skip_nonfinite=True).  Rank 1 alone writes Inf into its local gradient before
the all-reduce; the gate runs on the all-reduced G, which every rank holds alike, so BOTH ranks skip -- without a collective of the guard's own -- and the
next clean step leaves them with the same bits."""
import hashlib
import math
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
LT = dict(mlm=1, itm=1, t2i=1, cls=0)
T, IMG, B = 32, 64, 2


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


def _sha(*ts):
    h = hashlib.sha256()
    for t in ts:
        h.update(t.detach().cpu().numpy().tobytes())
    return h.hexdigest()


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
        opt = FusedAdamW(core, lr=1e-3, weight_decay=0.05, skip_nonfinite=True)
        scaler = BF16Scaler(skip_nonfinite=True)
        S = core.store
        poison = dict(on=False, hits=0)
        reduce_ = model._reduce

        def reduce_poisoned(store, lo, hi):
            """rank 1, poisoned step: Inf into the first trainable element of the first range that goes out -- its LOCAL gradient, before the all-reduce"""
            if poison["on"] and rank == 1 and poison["hits"] == 0:
                offs = sorted(store.offsets[n][0] for n, p in store.params.items() if p.requires_grad and lo <= store.offsets[n][0] < hi)
                if offs:
                    store.G[offs[0]] = float("inf")
                    poison["hits"] += 1
            return reduce_(store, lo, hi)

        model._reduce = reduce_poisoned
        batch = _batch(rank)

        def step():
            total, _ = train_step(model, batch, 1, True)
            opt.zero_grad()
            scaler(total, opt, clip_grad=1.0, parameters=model.parameters())
            torch.cuda.synchronize()
            assert S.pending_gate is None and S.pending_clip is None and S.pending_grad_scale == 1.0 and not S.scale_in_optimizer and not S.grad_works
            return _sha(S.P, opt._m, opt._v), float(scaler.last_grad_norm), (opt.applied_steps, opt.skipped_steps)

        s1, n1, c1 = step()
        poison["on"] = True
        s2, n2, c2 = step()
        poison["on"] = False
        s3, n3, c3 = step()
        q.put(dict(rank=rank, hits=poison["hits"], sha=[s1, s2, s3], norm=[n1, n2, n3], counts=[c1, c2, c3], finite=bool(torch.isfinite(S.P).all())))
    finally:
        dist.destroy_process_group()


def test_two_ranks_skip_together():
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
    assert r0["hits"] == 0 and r1["hits"] == 1                        # only rank 1 poisoned, and it did
    for r in res:
        assert r["counts"] == [(1, 0), (1, 1), (2, 1)], r             # both ranks skipped step 2, and only step 2
        assert r["sha"][1] == r["sha"][0], r                          # parameters and moments unchanged by the skipped step
        assert r["sha"][2] != r["sha"][1], r                          # the next clean step did step
        assert r["finite"]
        assert math.isfinite(r["norm"][0]) and not math.isfinite(r["norm"][1]) and math.isfinite(r["norm"][2]), r
    assert r0["sha"] == r1["sha"]                                     # equal across ranks after every step, bit for bit
    assert r0["norm"][0] == r1["norm"][0] and r0["norm"][2] == r1["norm"][2]
