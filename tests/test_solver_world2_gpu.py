"""World size 2 on the librccl stand-in (tests/test_comm_world2_gpu.py describes it): one norm-clipped general SGD step behind the
overlapped gradient exchange.  The gradient statistics must be those of the SUMMED gradients times 1 / world -- the order DDP and then
optimizer.step() give -- so both replicas end bitwise equal, and equal to a single process stepping on the summed gradients."""
import json
import os
import subprocess
import sys

import pytest

from test_comm_world2_gpu import FAKE_DIR, _free_port, build_fake_rccl

pytestmark = pytest.mark.gpu


def test_two_ranks_clip_on_the_summed_gradients(tmp_path):
    so = build_fake_rccl()
    port = _free_port()
    procs, outs = [], []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   AMP_RCCL_LIB=so, HSA_ENABLE_IPC_MODE_LEGACY="0")
        out = str(tmp_path / f"rank{rank}.json")
        log = open(tmp_path / f"rank{rank}.log", "w")
        procs.append((subprocess.Popen([sys.executable, os.path.join(FAKE_DIR, "rank_clip.py"), out], env=env, stdout=log, stderr=subprocess.STDOUT), log))
        outs.append(out)
    try:
        for p, _ in procs:
            p.wait(timeout=300)
    finally:
        for p, log in procs:
            if p.poll() is None:
                p.kill()                       # the exact children started above
                p.wait()
            log.close()
    logs = [open(tmp_path / f"rank{r}.log").read()[-3000:] for r in range(2)]
    assert all(p.returncode == 0 for p, _ in procs), "\n".join(logs)
    r0, r1 = [json.load(open(o)) for o in outs]
    for rep in (r0, r1):
        assert rep["scale"] == 0.5 and rep["exchanged"]
        assert rep["clipped"] >= 10 and rep["unclipped"] >= 10, (rep["clipped"], rep["unclipped"])
        assert rep["params"] == rep["solo_params"] and rep["momentum"] == rep["solo_momentum"], "the step behind the exchange != a single process on the summed gradients"
    assert r0["params"] == r1["params"] and r0["momentum"] == r1["momentum"] and r0["stats"] == r1["stats"], "the replicas diverged"
    assert "[fake_rccl]" not in logs[0] + logs[1], "the stand-in reported a sequence mismatch or a timeout"
