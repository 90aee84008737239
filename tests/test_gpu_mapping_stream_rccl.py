"""sharding.all_vs_all(mappings=True) through RCCL at world size 1 (modelled on test_gpu_rccl.py's
test_every_collective_through_rccl_at_world_size_one): one rank under torch.distributed.run, FA_FORCE_DIST=1, so the record
gather -- counts, then the padded payload -- runs through the library the multi-GPU run will use.  The mappings it returns
are the oracle's records (hit_mappings.expected) with global query ids."""
import os
import subprocess
import sys
import textwrap

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_all_vs_all_mappings_through_rccl_at_world_size_one(tmp_path):
    code = textwrap.dedent("""
        import os, sys, warnings
        sys.path.insert(0, %r)
        sys.path.insert(0, os.path.join(%r, "tests"))
        import numpy as np, torch, torch.distributed as dist
        torch.cuda.set_device(0)
        dist.init_process_group("nccl", device_id=torch.device("cuda", 0))
        assert dist.get_world_size() == 1 and dist.get_backend() == "nccl"
        import pyfastani_amd as pf
        from pyfastani_amd import sharding
        import hit_mappings as hm
        import mapping_stream as ms
        pf.set_device(0)
        assert sharding.collectives_on(1)
        inp = hm.inputs("contested")
        want = np.concatenate(hm.expected("contested")["maps"])
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            mapper = ms.new_mapper("contested")
            mapper.set_mapping_stage(64)
            batch = mapper.upload_genomes(inp["queries"])
            direct_rows, direct = batch.query_mappings()
            rows, maps = sharding.all_vs_all(mapper, inp["queries"], 0, 1, device="cuda", mappings=True)
            plain = sharding.all_vs_all(mapper, inp["queries"], 0, 1, device="cuda")
        assert maps.dtype == want.dtype and maps.tobytes() == want.tobytes(), (len(maps), len(want))
        assert maps.tobytes() == direct.tobytes() and rows.tobytes() == direct_rows.tobytes() == plain.tobytes()
        dist.barrier(); dist.destroy_process_group()
        open(os.path.join(%r, "ws1.ok"), "w").write("rccl_ranks: 1, backend: nccl, records: %%d" %% len(maps))
    """ % (ROOT, ROOT, str(tmp_path)))
    script = tmp_path / "worker_ws1.py"
    script.write_text(code)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=1", "--rdzv-backend=c10d",
           "--rdzv-endpoint=127.0.0.1:0", "--local-addr=127.0.0.1", str(script)]
    env = dict(os.environ, OMP_NUM_THREADS="1", HSA_ENABLE_IPC_MODE_LEGACY="0", FA_FORCE_DIST="1")
    res = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert res.returncode == 0, res.stdout + res.stderr
    assert (tmp_path / "ws1.ok").read_text().startswith("rccl_ranks: 1, backend: nccl")
