"""Dump every size query of the cached posterior (the two cache sizes and the predict, VJP, log-density,
leave-out, design and append workspace sizes of both families) over a grid, as JSON, for an A/B of
library builds.  User code sizes its buffers with these queries and the design workspace carries A from
one call into the next, so a host-layer change must leave every one of them as it was.  No GPU needed:
  python tools/posterior_sizes.py <libmfgp.so> OUT.json ;  cmp A.json B.json
The grid: both tile sizes; nlf 0 and 2; n and m on both sides of a tile edge (64 | 65) and of the 128-tile
switch of lo_layout and append_layout (4096 | 4097 at the 32-tile, 8192 | 8193 at the 64-tile); nstar 1,
32, 33 and the two values either side of post_chunk's whole-row threshold (batch * T * Ts >= 256) of each
problem; d 1 and 32; l 1 and 3; k 1 and APPEND_MAXK."""
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

NS = (10, 64, 65, 1000, 4096, 4097, 8192, 8193)
PS = (1, 3, 97)
APPEND_MAXK = 32


def nstars(nb, T, batch):
    """1, 32, 33 and the last nstar that cuts the rows / the first that keeps them whole."""
    ts = -(-256 // (batch * T))
    return sorted({1, 32, 33} | ({(ts - 1) * nb, (ts - 1) * nb + 1} if ts > 1 else set()))


def main(path, out):
    from multi_fidelity_gpflow_amd import _lib
    lib = _lib.load(path)
    h = C.c_void_p()
    assert lib.mfgp_create(0, C.byref(h)) == 0
    res = {}

    def q(name, *args):
        b = C.c_size_t(0)
        rc = getattr(lib, "mfgp_" + name)(h, *args, C.byref(b))
        assert rc == 0, (name, args, rc)
        res[f"{name}({','.join(map(str, args))})@{nb}"] = b.value

    for nb in (32, 64):
        assert lib.mfgp_set_tile(h, nb) == 0
        for d in (1, 32):
            for p in PS:
                for n in NS:
                    for nlf in (0, 2):
                        g = (nlf, n, p, d)
                        q("gpr_posterior_size", *g)
                        for ns in nstars(nb, -(-n // nb), 1):
                            q("gpr_posterior_predict_workspace_size", *g, ns)
                            q("gpr_posterior_logdens_workspace_size", *g, ns)
                            if nlf == 0:
                                q("gpr_posterior_predict_vjp_workspace_size", *g, ns)
                        for ng, nr in ((1, 1), (5, 9), (40, 1000)):
                            q("gpr_posterior_leave_out_workspace_size", *g, ng, nr)
                        for nref, ncand in ((0, 7), (5, 7), (300, 0), (1000, 500)):
                            q("gpr_posterior_design_workspace_size", *g, nref, ncand, 2)
                        for k in (1, APPEND_MAXK):
                            q("gpr_posterior_append_workspace_size", *g, k)
                    for l in (1, 3):
                        s = (n, l, p, d)   # m = n
                        q("svgp_posterior_size", *s)
                        for ns in nstars(nb, -(-n // nb), l):
                            for what in ("predict", "predict_vjp", "logdens"):
                                q(f"svgp_posterior_{what}_workspace_size", ns, *s)
    assert lib.mfgp_destroy(h) == 0
    with open(out, "w") as f:
        json.dump(res, f, indent=0, sort_keys=True)
    print(f"{len(res)} sizes written to {out}")


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
