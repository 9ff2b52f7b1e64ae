"""Child process of tests/test_gpu_grad_components.py: the fp64 LML gradient under one k_grad m-chunk.

  MFGP_GRAD_CHUNK=<chunk> python tests/_grad_chunk_worker.py <chunk> OUT.npz

The chunk is read once, when the library handle is created (mfgp_create), so each value needs a
process of its own.  The worker checks that the handle really took the value (mfgp_get_grad_chunk),
evaluates the chunk cases of tests/_grad_oracle.py (CHUNK_CASES: at tile 32 on the flow and on the
step schedule, at tile 64 on the step schedule) and saves [lml, gradient] of each leg."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import _grad_oracle as GR   # noqa: E402  (tests/ is the script's directory)


def main():
    chunk, out = int(sys.argv[1]), sys.argv[2]
    assert os.environ.get("MFGP_GRAD_CHUNK") == str(chunk), "the chunk goes in through the environment"
    from multi_fidelity_gpflow_amd.engine import Engine
    eng = Engine.get()
    got = eng.lib.mfgp_get_grad_chunk(eng.h)
    assert got == chunk == eng.mode()[3], f"the handle's k_grad chunk is {got}, not {chunk}"
    eng.set_tiny(False)
    res = {"chunk": np.array(got)}
    for name, nb in GR.CHUNK_CASES:
        X, Y, p = GR.case_data(name)
        Xd, Yd = torch.tensor(X, device=eng.device), torch.tensor(Y, device=eng.device)
        th = torch.tensor(GR.theta_vector(p), dtype=torch.float64, device=eng.device)
        eng.set_tile(nb)
        for flow in ((True, False) if nb == 32 else (False,)):
            eng.set_flow(flow, any_size=True)
            assert eng.flow_runs(X.shape[0]) == flow
            o, info = eng.gpr_lml(Xd, Yd, th, want_grad=True)
            torch.cuda.synchronize()
            assert int(info.item()) == 0, (name, nb, flow, int(info.item()))
            res[f"{name}_nb{nb}_{'flow' if flow else 'steps'}"] = o.cpu().numpy().copy()
    np.savez(out, **res)
    print(f"chunk {chunk}: ok", flush=True)


if __name__ == "__main__":
    main()
