"""Section 8(e): the N>1 path on CPU - world_size 2, gloo backend, 127.0.0.1 rendezvous.
Each rank inspects image_paths[r::2] with a mock backend, one all_gather exchanges the records,
every rank returns the full input-ordered result."""
import json
import os
import socket
import sys

import numpy as np
import pytest
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, paths, outdir):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from vision_inspection_system_amd import config as C
    from vision_inspection_system_amd.batch import gather_records, run_multi_image_inspection
    C.set_config(C.Config(vlm_inspector_provider="mock", vlm_auditor_provider="mock"))
    # raw collective: ragged payloads, one rank empty
    recs = gather_records([{"r": rank, "i": i, "pad": "x" * (50 * rank)} for i in range(3 * rank)], world)
    assert [(r["r"], r["i"]) for r in recs] == [(1, 0), (1, 1), (1, 2)]

    def fake_inspect(image_path, criticality, domain, user_notes):
        if image_path.endswith("bad.png"):
            raise RuntimeError("decode error")
        return {"inspector_result": {"who": rank}, "auditor_result": {}, "safety_verdict": {"verdict": "SAFE"},
                "consensus": {"combined_defects": [{"safety_impact": "COSMETIC"}]}, "processing_time": 0.01}
    out = run_multi_image_inspection(paths, session_id=None, _inspect=fake_inspect)
    with open(os.path.join(outdir, f"rank{rank}.json"), "w") as f:
        json.dump(out, f, default=str)
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_batch(tmp_path):
    paths = [str(tmp_path / n) for n in ("a.png", "b.png", "bad.png", "c.png", "d.png")]
    port = _free_port()
    mp.spawn(_worker, args=(2, port, paths, str(tmp_path)), nprocs=2, join=True)
    r0 = json.load(open(tmp_path / "rank0.json"))
    r1 = json.load(open(tmp_path / "rank1.json"))
    assert r0["image_results"] == r1["image_results"] and r0["session_id"] == r1["session_id"]
    res = r0["image_results"]
    assert [v["image_path"] for v in res.values()] == paths          # input order restored
    assert [v.get("completed") for v in res.values()] == [True, True, False, True, True]
    # rank r handled paths[r::2]
    assert [v["inspector_result"]["who"] for v in res.values() if v["completed"]] == [0, 1, 1, 0]
    sr = r0["session_results"]
    assert sr["total_images"] == 5 and sr["completed_images"] == 4 and sr["failed_images"] == 1
    assert sr["aggregate_verdict"] == "SAFE" and sr["cosmetic_defects"] == 4
    assert res[list(res)[2]]["error"] == "decode error"


def _worker_failure(rank, world, port, paths, outdir, mode):
    """mode 'dead': the last rank exits before the exchange; 'late': it arrives after the others gave up."""
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      VIS_RANK_TIMEOUT_S="5")      # generous: a loaded CI host must not turn a live rank into a "dead" one
    import time
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from vision_inspection_system_amd import config as C
    from vision_inspection_system_amd.batch import run_multi_image_inspection
    C.set_config(C.Config(vlm_inspector_provider="mock", vlm_auditor_provider="mock"))
    dist.barrier()      # every rank has finished its imports (seconds apart on a cold page cache): the 5 s below time the exchange only
    if rank == world - 1:
        if mode == "dead":
            os._exit(0)

    def fake_inspect(image_path, criticality, domain, user_notes):
        if rank == world - 1 and mode == "late":
            time.sleep(3.5)          # rank 2's two images x 3.5 s > the 5 s the others wait
        return {"inspector_result": {"who": rank}, "auditor_result": {}, "safety_verdict": {"verdict": "SAFE"},
                "consensus": {"combined_defects": []}, "processing_time": 0.01}
    t0 = time.monotonic()
    out = run_multi_image_inspection(paths, session_id="sess", _inspect=fake_inspect)
    out["_elapsed"] = time.monotonic() - t0
    with open(os.path.join(outdir, f"rank{rank}.json"), "w") as f:
        json.dump(out, f, default=str)
    # no barrier / destroy: the default group is unusable once a rank is gone, which is the point of the test
    if rank == 0:     # rank 0 hosts the rendezvous store: stay until every other reporting rank has read it
        others = range(1, world if mode == "late" else world - 1)
        for _ in range(200):
            if all(os.path.exists(os.path.join(outdir, f"rank{r}.json")) for r in others):
                break
            time.sleep(0.1)
    os._exit(0)


@pytest.mark.parametrize("mode", ["dead", "late"])
def test_rank_failure_is_a_result_not_a_hang(tmp_path, mode):
    """SURVEY section 5 / graph.py:349-357: a rank that dies (or hangs past VIS_RANK_TIMEOUT_S) turns into
    completed=False records for ITS images on every surviving rank; nobody blocks in a collective."""
    world = 3
    paths = [str(tmp_path / f"img{i}.png") for i in range(8)]
    port = _free_port()
    mp.spawn(_worker_failure, args=(world, port, paths, str(tmp_path), mode), nprocs=world, join=True)
    outs = [json.load(open(tmp_path / f"rank{r}.json")) for r in range(world) if (tmp_path / f"rank{r}.json").exists()]
    assert len(outs) == (2 if mode == "dead" else 3)
    for o in outs[:2]:
        assert o["_elapsed"] < 45
        res = o["image_results"]
        assert [v["image_path"] for v in res.values()] == paths
        done = [v.get("completed") for v in res.values()]
        assert done == [i % world != world - 1 for i in range(8)]
        bad = [v for v in res.values() if not v["completed"]]
        assert all("rank 2 did not report" in v["error"] for v in bad)
        assert o["session_results"]["failed_images"] == len(bad) == 2
    assert outs[0]["image_results"] == outs[1]["image_results"]
    if mode == "late":       # the late rank sees the same verdict about itself
        assert outs[2]["image_results"] == outs[0]["image_results"]


def _worker_degraded(rank, world, port, outdir):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      VIS_RANK_TIMEOUT_S="5")
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from vision_inspection_system_amd import batch as B
    calls = []
    real = B._all_gather_bytes
    B._all_gather_bytes = lambda d, p: (calls.append(1), real(d, p))[1]
    dist.barrier()      # imports done on every rank before anything is timed against VIS_RANK_TIMEOUT_S
    first, miss0 = B.gather_records_ft([{"r": rank, "n": 0}])            # clean: the collective
    if rank == 1:
        B._DEGRADED[0] = True       # what the except branch leaves behind when an exchange raised on this rank only
    second, miss1 = B.gather_records_ft([{"r": rank, "n": 1}])           # rank 1 votes degraded -> everyone uses the store
    third, miss2 = B.gather_records_ft([{"r": rank, "n": 2}])            # and stays there
    with open(os.path.join(outdir, f"rank{rank}.json"), "w") as f:
        json.dump({"first": first, "second": second, "third": third, "missing": [miss0, miss1, miss2],
                   "collectives": len(calls), "degraded": B._DEGRADED[0]}, f)
    dist.barrier()
    dist.destroy_process_group()


def test_exchange_mode_is_voted_not_local(tmp_path):
    """a rank whose exchange failed must not take the store path alone while the others enter the
    collective.  The mode is published by rank 0 from every rank's vote; all ranks follow it."""
    port = _free_port()
    mp.spawn(_worker_degraded, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    r0 = json.load(open(tmp_path / "rank0.json"))
    r1 = json.load(open(tmp_path / "rank1.json"))
    for k in ("first", "second", "third"):
        assert r0[k] == r1[k] and [x["r"] for x in r0[k]] == [0, 1]
    assert r0["missing"] == r1["missing"] == [[], [], []]
    assert r0["collectives"] == r1["collectives"] == 1            # only the first exchange used the default group
    assert r0["degraded"] and r1["degraded"]
