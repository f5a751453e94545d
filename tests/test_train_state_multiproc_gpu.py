"""TrainEngine.state_dict() / load_state_dict() over two data-parallel ranks (gloo, both on cuda:0): rank 0 saves after three
steps, BOTH ranks load that one file into fresh engines and train three more -- master, moments and step state are bit-identical
across the ranks and equal to an uninterrupted six-step pair of ranks; a state written by a single process is refused on both."""
import os
import socket
import sys
import time

import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER_LIMIT_S = 240          # per worker: four engines x a few tiny steps + the process group (torch's import is most of it)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _build(seed=0):
    sys.path.insert(0, os.path.join(ROOT, "kindergarten-vq-vae_amd"))
    from models.shelgon3.Shelgon import Shelgon
    from models.shelgon3.VectorQuantizer import VectorQuantizer
    torch.manual_seed(seed)
    vq = VectorQuantizer(32, 128, 0.25, vq_codebook_init_values=torch.randn(32, 128))
    vq.materialize_min_encodings = False
    return Shelgon("kvq-bert-tiny", vq, "kvq-bert-tiny", None, compute_dtype=torch.float32).cuda().train()      # dropout on


def _data(step):
    g = torch.Generator().manual_seed(30 + step)
    ids = torch.randint(1000, 2000, (8, 16), generator=g)
    lens = torch.randint(3, 17, (8,), generator=g)
    ids = ids * (torch.arange(16)[None] < lens[:, None])
    return ids.cuda(), (ids != 0).long().cuda()


def _same_on_all_ranks(t):
    import torch.distributed as dist
    raw = t.detach().contiguous().reshape(-1)
    raw = raw.view(torch.int32 if raw.element_size() == 4 else torch.int64).cpu()
    hi, lo = raw.clone(), raw.clone()
    dist.all_reduce(hi, op=dist.ReduceOp.MAX)
    dist.all_reduce(lo, op=dist.ReduceOp.MIN)
    return bool(torch.equal(hi, lo))


def _words(eng):
    torch.cuda.synchronize()
    return {"master": eng.flat.master.clone(), "m": eng.flat.m.clone(), "v": eng.flat.v.clone(), "state": eng._state.clone(),
            "codebook": eng.E.data.clone(), "codebook_m": eng.aux[0]["m"].clone()}


def _worker(rank, world, port, tmp):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0")
    for name in ("KVQ_MAX_GRAD_NORM", "KVQ_GRAD_ACCUM", "KVQ_VQ_REVIVE_AFTER", "KVQ_FP8"):
        os.environ.pop(name, None)
    sys.path.insert(0, os.path.join(ROOT, "kindergarten-vq-vae_amd"))
    import torch.distributed as dist
    from kvq import ddp
    from kvq._ffi import KvqError
    from kvq.engine import TrainEngine
    torch.cuda.set_device(0)
    ddp.init_distributed("gloo")
    half = slice(rank * 4, rank * 4 + 4)

    def engine(seed):
        model = _build(seed)
        ddp.broadcast_parameters(model)
        eng = TrainEngine(model, lr=1e-3, bucket_mib=0)             # bucket_mib=0: many chunks, a cut inside the buffer
        assert eng.world == 2 and eng._dp
        return eng

    def steps(eng, lo, hi):
        for s in range(lo, hi + 1):
            ids, mask = _data(s)
            eng.train_step(ids[half], mask[half])

    report = {}
    whole = engine(0)                                               # the uninterrupted pair: six steps
    steps(whole, 1, 6)
    want = _words(whole)
    first = engine(0)                                               # the pair that is cut off after three
    steps(first, 1, 3)
    path = os.path.join(tmp, "pair_state.pth")
    if rank == 0:                                                   # rank 0 writes, behind a barrier every rank reads the same file
        torch.save({"engine": first.state_dict(), "model": first.model.state_dict()}, path + ".tmp")
        os.replace(path + ".tmp", path)
    dist.barrier()
    report["readable"] = ddp.readable_everywhere(path)
    blob = torch.load(path, weights_only=True)
    del first
    resumed = engine(1234 + rank)                                   # fresh weights (rank 0's, after the broadcast) -- all overwritten
    resumed.model.load_state_dict(blob["model"])
    resumed.load_state_dict(blob["engine"])
    report["step_after_load"] = resumed.step_count
    steps(resumed, 4, 6)
    got = _words(resumed)
    report["same_across_ranks"] = {k: _same_on_all_ranks(v) for k, v in got.items()}
    report["equal_to_uninterrupted"] = {k: bool(torch.equal(got[k].view(torch.int32) if got[k].element_size() == 4 else got[k],
                                                            want[k].view(torch.int32) if want[k].element_size() == 4 else want[k]))
                                        for k in got}
    report["graphs"] = (len(whole._graphs), len(resumed._graphs))
    # a state of world = 1 (written by the parent process, no process group there) is refused on both ranks, nothing written
    single = torch.load(os.path.join(tmp, "single_state.pth"), weights_only=True)
    before = _words(resumed)
    try:
        resumed.load_state_dict(single)
        report["refusal"] = None
    except KvqError as e:
        report["refusal"] = str(e)
    after = _words(resumed)
    report["refusal_wrote_nothing"] = all(torch.equal(before[k], after[k]) for k in before)
    torch.save(report, os.path.join(tmp, f"report{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def _spawn_with_limit(fn, args, nprocs, limit_s):
    """mp.spawn whose workers are killed, and the test failed, when they are not done after limit_s seconds."""
    ctx = mp.spawn(fn, args=args, nprocs=nprocs, join=False)
    deadline = time.monotonic() + limit_s
    while not ctx.join(timeout=5.0):
        if time.monotonic() > deadline:
            for p in ctx.processes:
                if p.is_alive():
                    p.kill()
            pytest.fail(f"a data-parallel worker was not done after {limit_s} s")


def test_two_ranks_resume_from_rank_zeros_file(tmp_path):
    from kvq.engine import TrainEngine
    solo = TrainEngine(_build(0), lr=1e-3, bucket_mib=0)
    assert solo.world == 1
    ids, mask = _data(1)
    solo.train_step(ids, mask)
    st = solo.state_dict()
    assert st["fingerprint"]["world"] == 1
    torch.save(st, str(tmp_path / "single_state.pth"))
    del solo, st
    _spawn_with_limit(_worker, (2, _free_port(), str(tmp_path)), 2, WORKER_LIMIT_S)
    for rank in (0, 1):
        rep = torch.load(str(tmp_path / f"report{rank}.pt"))
        print(rank, rep)
        assert rep["readable"] is True and rep["step_after_load"] == 3
        assert all(rep["same_across_ranks"].values()), rep["same_across_ranks"]
        assert all(rep["equal_to_uninterrupted"].values()), rep["equal_to_uninterrupted"]
        assert rep["graphs"] == (1, 1)                               # both pairs ended up replaying
        assert rep["refusal"] is not None and "fingerprint.world" in rep["refusal"] and "state 1, engine 2" in rep["refusal"]
        assert rep["refusal_wrote_nothing"]
