"""Return codes of the GPR, graph-kernel, predict, fp32, potrf and fence entries of libmfgp.so for bad
arguments, as a table: each case changes one or two arguments of a valid call and names the code that
comes back.  The doubly-wrong cases pin the order of the checks (handle, then d, then nlf / dtype,
then sizes and pointers; nstar == 0 returns MFGP_OK between the two pointer checks of a predict).
No case passes validation with its stand-in pointers, so nothing is launched and no GPU is needed.
The cached-posterior entries have a table of their own below (POST): their valid calls pass validation
and stop at MFGP_ERR_WORKSPACE, before any launch, on buffers of zero bytes."""
import ctypes as C

import pytest
import torch

OK, ARG, DIM = 0, -1, -4
MAX_LF = 4
J = 0x1000   # a non-null stand-in: every case fails validation (or returns early) before it is read
F64, F32 = 0, 1


@pytest.fixture(scope="module")
def lib():
    from multi_fidelity_gpflow_amd import _lib
    from multi_fidelity_gpflow_amd.build import build_lib
    build_lib()
    return _lib.load()


@pytest.fixture(scope="module")
def h(lib):
    hp = C.c_void_p()
    assert lib.mfgp_create(0, C.byref(hp)) == 0
    yield hp
    assert lib.mfgp_destroy(hp) == 0


def _train(pre=(), post=()):
    return list(pre) + [("n", 10), ("p", 2), ("d", 3), ("X", J), ("ldx", 4), ("Y", J), ("ldy", 2)] + list(post)


_ADAM = [("theta", J), ("u", J), ("m", J), ("v", J), ("trainable", J), ("tie", J), ("step", J), ("lr", 0.1),
         ("b1", 0.9), ("b2", 0.999), ("eps", 1e-7), ("loss_hist", J), ("ws", J), ("ws_bytes", 0), ("out", J),
         ("info", J)]
_LML = [("theta", J), ("want_grad", 1), ("ws", J), ("ws_bytes", 0), ("out", J), ("info", J)]
_PRED = [("Xs", J), ("ldxs", 4), ("theta", J), ("ws", J), ("ws_bytes", 0), ("mean", J), ("ldm", 2), ("var", J)]


def _pred(pre=(), cov=False):
    a = list(pre) + [("n", 10), ("p", 2), ("d", 3), ("nstar", 5), ("X", J), ("ldx", 4), ("Y", J), ("ldy", 2)] + _PRED
    return a + ([("cov", J), ("ldc", 5)] if cov else []) + [("info", J)]


_PH = [("theta", J), ("ws", J), ("ws_bytes", 0), ("out", J), ("info", J), ("ms", J)]
DT, LF, LF0 = [("dtype", F32)], [("nlf", 1)], [("nlf", 0)]

# entry -> the arguments after the handle, in order, with values of a valid call
ENTRIES = {
    "mfgp_gpr_workspace_size": [("n", 10), ("p", 2), ("d", 3), ("bytes", J)],
    "mfgp_gmf_gpr_workspace_size": LF + [("n", 10), ("p", 2), ("d", 3), ("bytes", J)],
    "mfgp_gpr_workspace_size_ex": DT + [("n", 10), ("p", 2), ("d", 3), ("bytes", J)],
    "mfgp_gpr_flow_trace": [("n", 10), ("p", 2), ("d", 3), ("offset", J), ("count", J)],
    "mfgp_gpr_lml": _train(post=_LML),
    "mfgp_gmf_gpr_lml": _train(LF, _LML),
    "mfgp_gpr_lml_ex": _train(DT, _LML),
    "mfgp_gpr_adam_step": _train(post=_ADAM),
    "mfgp_gpr_adam_steps": _train(post=_ADAM + [("nsteps", 2)]),
    "mfgp_gpr_adam_step_ex": _train(DT, _ADAM),
    "mfgp_gpr_lml_phase_times": _train(post=_PH),
    "mfgp_gpr_phase_times_ex": _train(DT, _PH + [("flops", J), ("launches", J), ("nphase", 5)]),
    "mfgp_gpr_predict_workspace_size": [("n", 10), ("p", 2), ("d", 3), ("nstar", 5), ("bytes", J)],
    "mfgp_gmf_gpr_predict_workspace_size": LF + [("n", 10), ("p", 2), ("d", 3), ("nstar", 5), ("bytes", J)],
    "mfgp_gpr_predict_cov_workspace_size": LF0 + [("n", 10), ("p", 2), ("d", 3), ("nstar", 5), ("bytes", J)],
    "mfgp_gpr_predict_workspace_size_ex": DT + [("n", 10), ("p", 2), ("d", 3), ("nstar", 5), ("bytes", J)],
    "mfgp_gpr_predict_cov_workspace_size_ex": DT + LF0 + [("n", 10), ("p", 2), ("d", 3), ("nstar", 5), ("bytes", J)],
    "mfgp_gpr_predict": _pred(),
    "mfgp_gmf_gpr_predict": _pred(LF),
    "mfgp_gpr_predict_cov": _pred(LF0, cov=True),
    "mfgp_gpr_predict_ex": _pred(DT),
    "mfgp_gpr_predict_cov_ex": _pred(DT + LF0, cov=True),
    "mfgp_potrf_inv_workspace_size": [("n", 33), ("batch", 2), ("bytes", J)],
    "mfgp_potrf_inv": [("n", 33), ("batch", 2), ("A", J), ("lda", 33), ("sA", 33 * 33), ("ws", J), ("ws_bytes", 0),
                       ("Linv", J), ("ldl", 33), ("sL", 33 * 33), ("ldiag", J), ("info", J)],
    "mfgp_flow_fence": [("op", 0)],
}
OPTIONAL = {"tie", "ldiag", "flops", "launches"}   # pointers that may be NULL
SIZE_ONLY = {k for k in ENTRIES if k.endswith("_workspace_size") or k.endswith("_workspace_size_ex")} | {
    "mfgp_gpr_flow_trace", "mfgp_flow_fence"}
# pointers a predict entry checks only after its nstar == 0 return
PRED_OUT = {"Xs", "mean", "var", "cov"}


# outputs an entry may write although it returns an error (mfgp_gpr_phase_times_ex fills ms / flops /
# launches after its fp64 call), and the size queries' results: real memory instead of the stand-in
_BUF = (C.c_double * 64)()
LIVE = {"bytes", "offset", "count", "ms", "flops", "launches"}


def _args(name):
    return ENTRIES[name] if name in ENTRIES else POST[name]


def _call(lib, h, name, change, handle=True):
    fn = getattr(lib, name)
    args = []
    for (k, v), ty in zip(_args(name), fn.argtypes[1:]):
        v = change.get(k, v)
        if v == J and k in LIVE:
            v = C.addressof(_BUF)
        if isinstance(v, int) and hasattr(ty, "contents"):
            v = C.cast(v, ty)
        args.append(v)
    for k in change:
        assert k in dict(_args(name)), (name, k)
    return fn(h if handle else None, *args)


def _has(name, arg):
    return arg in dict(_args(name))


def _cases(name):
    """(change, expected code, handle given) for one entry."""
    f32 = _has(name, "dtype")
    gmf = name.startswith("mfgp_gmf_")
    has_d = _has(name, "d")
    out = [({}, ARG, False)]
    if name == "mfgp_flow_fence":
        return out + [({"op": 2}, ARG, True), ({"op": -1}, ARG, True)]
    if has_d:
        # d before everything but the handle -- except mfgp_gpr_predict_cov_workspace_size_ex, which
        # checks the dtype first and leaves d to the entry it dispatches to
        covsz = name == "mfgp_gpr_predict_cov_workspace_size_ex"
        out += [({"d": 0}, ARG, False), ({"d": 0}, DIM, True), ({"d": 33}, DIM, True),
                ({"d": 0, "n": 0}, DIM, True), ({"d": 33, "p": 0}, DIM, True)]
        if gmf:
            out += [({"d": 0, "nlf": 0}, DIM, True), ({"d": 33, "nlf": MAX_LF + 1}, DIM, True)]
        if f32:
            out += [({"d": 0, "dtype": 7}, ARG if covsz else DIM, True), ({"dtype": 7}, ARG, True),
                    ({"dtype": -1}, ARG, True), ({"d": 0, "dtype": F64}, DIM, True)]
            if covsz:
                out += [({"d": 0, "nlf": 1}, ARG, True), ({"nlf": 1}, ARG, True),
                        ({"nlf": 1, "dtype": F64, "d": 33}, DIM, True), ({"nlf": -1, "dtype": F64}, ARG, True)]
        if gmf:
            out += [({"nlf": 0}, ARG, True), ({"nlf": MAX_LF + 1}, ARG, True), ({"nlf": 0, "n": 0}, ARG, True)]
        if "predict_cov" in name and not covsz:
            out += [({"nlf": -1}, ARG, True), ({"nlf": MAX_LF + 1}, ARG, True), ({"nlf": -1, "d": 0}, DIM, True)]
            if f32:
                out += [({"nlf": 1}, ARG, True), ({"nlf": -1, "dtype": F64}, ARG, True),
                        ({"nlf": MAX_LF + 1, "dtype": F64, "nstar": 0}, ARG, True)]
    out += [({"n": 0}, ARG, True)]
    if _has(name, "p"):
        out += [({"p": 0}, ARG, True)]
    if _has(name, "batch"):
        out += [({"batch": 0}, ARG, True)]
    if _has(name, "nstar"):
        out += [({"nstar": -1}, ARG, True), ({"nstar": -1, "d": 0}, DIM, True)]
    if _has(name, "nsteps"):
        out += [({"nsteps": -1}, ARG, True), ({"nsteps": -1, "d": 0}, DIM, True), ({"nsteps": -1, "X": None}, ARG, True),
                ({"nsteps": 0, "X": None}, ARG, True)]
    if _has(name, "nphase"):   # ms / nphase come before the dtype dispatch
        out += [({"nphase": 0}, ARG, True), ({"ms": None, "dtype": F64}, ARG, True), ({"nphase": 0, "d": 0}, DIM, True),
                ({"nphase": 0, "dtype": 7}, ARG, True)]
    return out


def _pointer_cases(name):
    """Each required pointer NULL in turn, the predict entries' nstar == 0 return, and the leading-dimension checks."""
    out = []
    pred = _has(name, "Xs")
    for k, v in ENTRIES[name]:
        if v == J and k not in OPTIONAL:
            out.append(({k: None}, ARG))
            for dt in ((F64,) if _has(name, "dtype") else ()):
                if not (name == "mfgp_gpr_phase_times_ex" and k in ("flops", "launches")):
                    out.append(({k: None, "dtype": dt}, ARG))
            if pred:   # nstar == 0 returns MFGP_OK after the first pointer check, before the second
                out.append(({k: None, "nstar": 0}, OK if k in PRED_OUT else ARG))
    for k in OPTIONAL:
        if _has(name, k):
            out.append(({k: None, "n": 0}, ARG))
    if pred:
        none_out = {k: None for k in PRED_OUT if _has(name, k)}
        out += [(dict(none_out, nstar=0), OK), (dict(none_out, nstar=0, n=0), ARG), (dict(none_out, nstar=0, d=0), DIM)]
        if _has(name, "dtype"):
            out += [(dict(none_out, nstar=0, dtype=F64), OK), (dict(none_out, nstar=0, ldx=1), OK)]
        if _has(name, "ldc"):
            out += [({"ldc": 4}, ARG), ({"ldc": 4, "nstar": 0}, OK), ({"ldc": 0, "nstar": 0, "cov": None}, OK)]
            if _has(name, "dtype"):
                out += [({"ldc": 4, "dtype": F64}, ARG)]
    if _has(name, "dtype") and _has(name, "ldx") and name != "mfgp_gpr_phase_times_ex":
        out += [({"ldx": 3}, ARG), ({"ldy": 1}, ARG), ({"ldx": 3, "d": 33}, DIM)]
        if pred:
            out += [({"ldxs": 3}, ARG), ({"ldm": 1}, ARG), ({"ldxs": 3, "nstar": 0}, OK)]
    return out


def _show(name, change, handle):
    return f"{name}({'h' if handle else 'NULL'}, {change})"


@pytest.mark.parametrize("name", sorted(SIZE_ONLY))
def test_size_entry_codes(lib, h, name):
    for change, want, handle in _cases(name):
        assert _call(lib, h, name, change, handle) == want, _show(name, change, handle)
    for k in ("bytes", "offset", "count"):
        if _has(name, k):
            assert _call(lib, h, name, {k: None}) == ARG, _show(name, {k: None}, True)
            if _has(name, "d"):
                assert _call(lib, h, name, {k: None, "d": 0}) == DIM, _show(name, {k: None, "d": 0}, True)
    if _has(name, "nstar"):   # a size query takes nstar == 0
        assert _call(lib, h, name, {"nstar": 0}) == OK, _show(name, {"nstar": 0}, True)


@pytest.mark.skipif(torch.cuda.is_available(), reason="null-pointer calls are a host-only check")
@pytest.mark.parametrize("name", sorted(set(ENTRIES) - SIZE_ONLY))
def test_compute_entry_codes(lib, h, name):
    for change, want, handle in _cases(name):
        assert _call(lib, h, name, change, handle) == want, _show(name, change, handle)
    for change, want in _pointer_cases(name):
        assert _call(lib, h, name, change) == want, _show(name, change, True)


# ---- the cached posterior (mfgp_gpr_posterior_* / mfgp_svgp_posterior_*).  Every valid call has
# cache_bytes = ws_bytes = 0, so a call that passes validation returns MFGP_ERR_WORKSPACE before any
# launch.  The order of these entries' checks is their own, not the GPR convention's: the cases
# are written out per entry.
WS = -2
J2 = 0x2000   # a second stand-in (mfgp_gpr_posterior_append wants out_cache != cache)
DESIGN_MAXQ = APPEND_MAXK = LO_W = 32
_G = [("nlf", 0), ("n", 10), ("p", 2), ("d", 3)]
_GQ = _G + [("nstar", 5), ("cache", J), ("cache_bytes", 0), ("Xs", J), ("ldxs", 4), ("ws", J), ("ws_bytes", 0),
            ("mean", J), ("ldm", 2), ("var", J)]
_S = [("m", 40), ("l", 2), ("p", 3), ("d", 3)]
_SQ = [("nstar", 5)] + _S + [("mixed", 1), ("cache", J), ("cache_bytes", 0), ("Xs", J), ("ldxs", 4), ("ws", J),
                             ("ws_bytes", 0), ("f_mu", J), ("f_var", J)]
_VJP = [("gmean", J), ("ldgm", 3), ("gvar", J), ("gX", J), ("ldgx", 4)]
_DENS = [("Y", J), ("y_rs", 3), ("obs_var", J), ("ov_rs", 3), ("obs_cov", None), ("ldc", 0), ("logp", J), ("gX", J),
         ("ldgx", 4), ("info", J)]
_DES = _G + [("cache", J), ("cache_bytes", 0), ("Xall", J), ("ldx", 4), ("nref", 5), ("ncand", 7)]
POST = {
    "mfgp_gpr_posterior_size": _G + [("bytes", J)],
    "mfgp_gpr_posterior_build": _G + [("X", J), ("ldx", 4), ("Y", J), ("ldy", 2), ("theta", J), ("ws", J), ("ws_bytes", 0),
                                      ("cache", J), ("cache_bytes", 0), ("info", J)],
    "mfgp_gpr_posterior_predict_workspace_size": _G + [("nstar", 5), ("bytes", J)],
    "mfgp_gpr_posterior_predict": _GQ + [("cov", None), ("ldc", 0)],
    "mfgp_gpr_posterior_predict_vjp_workspace_size": _G + [("nstar", 5), ("bytes", J)],
    "mfgp_gpr_posterior_predict_vjp": _GQ + [("gmean", J), ("ldgm", 2)] + _VJP[2:],
    "mfgp_gpr_posterior_logdens_workspace_size": _G + [("nstar", 5), ("bytes", J)],
    "mfgp_gpr_posterior_logdens": _GQ + [("Y", J), ("y_rs", 2), ("obs_var", J), ("ov_rs", 2)] + _DENS[4:],
    "mfgp_gpr_posterior_leave_out_workspace_size": _G + [("ngroups", 3), ("nrows", 5), ("bytes", J)],
    "mfgp_gpr_posterior_leave_out": _G + [("cache", J), ("cache_bytes", 0), ("ngroups", 3), ("offsets", J), ("rows", J),
                                          ("nrows", 5), ("gmax", 2), ("ws", J), ("ws_bytes", 0), ("resid", J),
                                          ("ldr", 2), ("cov", J), ("ldc", 2), ("logdens", J), ("info", J)],
    "mfgp_gpr_posterior_design_workspace_size": _G + [("nref", 5), ("ncand", 7), ("qmax", 2), ("bytes", J)],
    "mfgp_gpr_posterior_design_score": _DES + [("w", J), ("E", J), ("ldE", 12), ("k", 1), ("ws", J), ("ws_bytes", 0),
                                               ("score", J), ("refresh", 0)],
    "mfgp_gpr_posterior_design_append": _DES + [("ws", J), ("ws_bytes", 0), ("pick", J), ("E", J), ("ldE", 12), ("k", 1)],
    "mfgp_gpr_posterior_append_workspace_size": _G + [("k", 3), ("bytes", J)],
    "mfgp_gpr_posterior_append": _G + [("k", 3), ("cache", J), ("cache_bytes", 0), ("Xadd", J), ("ldxa", 4), ("Yadd", J),
                                       ("ldya", 2), ("ws", J), ("ws_bytes", 0), ("out_cache", J2), ("out_bytes", 0),
                                       ("mean_add", J), ("ldm", 2), ("info", J)],
    "mfgp_svgp_posterior_size": _S + [("bytes", J)],
    "mfgp_svgp_posterior_build": _S + [("Z", J), ("ldz", 4), ("thetas", J), ("q_mu", J), ("q_sqrt", J), ("W", J),
                                       ("jitter", 1e-6), ("ws", J), ("ws_bytes", 0), ("cache", J), ("cache_bytes", 0),
                                       ("info", J)],
    "mfgp_svgp_posterior_predict_workspace_size": [("nstar", 5)] + _S + [("bytes", J)],
    "mfgp_svgp_posterior_predict": _SQ,
    "mfgp_svgp_posterior_predict_vjp_workspace_size": [("nstar", 5)] + _S + [("bytes", J)],
    "mfgp_svgp_posterior_predict_vjp": _SQ + _VJP,
    "mfgp_svgp_posterior_logdens_workspace_size": [("nstar", 5)] + _S + [("bytes", J)],
    "mfgp_svgp_posterior_logdens": _SQ + _DENS,
}
# pointers that may be NULL in a valid call, and where the valid call of an entry needs one of them all the same
POST_OPTIONAL = {"cov", "gmean", "gvar", "obs_var", "obs_cov", "w", "Yadd", "mean_add", "W", "gX"}
POST_REQUIRED = {("mfgp_gpr_posterior_predict_vjp", "gX"), ("mfgp_svgp_posterior_predict_vjp", "gX"),
                 ("mfgp_svgp_posterior_build", "W")}   # (l != p in the valid call)
POST_SIZE = {k for k in POST if k.endswith("_size")}


def _all_null(name):
    return {k: None for k, v in POST[name] if v in (J, J2)}


def _post_common(name):
    """(change, code, handle given): the handle, then d, before anything else; then the sizes."""
    gpr = name.startswith("mfgp_gpr_")
    bad = {"nlf": MAX_LF + 1} if gpr else {"m": 0}
    out = [({}, ARG, False), ({"d": 0}, ARG, False), ({"d": 0}, DIM, True), ({"d": 33}, DIM, True),
           (dict(bad, d=0), DIM, True), ({"d": 33, "p": 0}, DIM, True), (dict(_all_null(name), d=0), DIM, True)]
    for k in (("n", "p") if gpr else ("m", "l", "p")):
        out += [({k: 0}, ARG, True)]
    if gpr:
        out += [({"nlf": -1}, ARG, True), ({"nlf": MAX_LF + 1}, ARG, True)]
    if _has(name, "nstar"):
        out += [({"nstar": -1}, ARG, True), ({"nstar": -1, "d": 0}, DIM, True), ({"nstar": 0, "d": 33}, DIM, True)]
    return out


def _post_pointers(name, early=None):
    """Each required pointer NULL in turn -> MFGP_ERR_ARG, each optional one -> as the valid call.  early: a
    change that makes the entry return MFGP_OK before its pointer check, which then sees no pointer at all."""
    out = []
    for k, v in POST[name]:
        if v in (J, J2) and k not in LIVE:
            opt = k in POST_OPTIONAL and (name, k) not in POST_REQUIRED
            out.append(({k: None}, WS if opt else ARG))
            if early:
                out.append((dict(early, **{k: None}), OK))
    if early:
        out += [(early, OK), (dict(_all_null(name), **early), OK), (dict(early, d=0), DIM)]
    return out


# what each entry adds to the common cases: (change, code)
_NS0 = {"nstar": 0}
POST_CASES = {
    "mfgp_gpr_posterior_size": [({}, OK)],
    "mfgp_gpr_posterior_build": [({}, WS), ({"ldx": 3}, ARG), ({"ldy": 1}, ARG), ({"nlf": 2}, WS)],
    # the size queries reject nstar == 0 (the GPR predict size queries take it)
    "mfgp_gpr_posterior_predict_workspace_size": [({}, OK), (_NS0, ARG), ({"nlf": 2}, OK)],
    # no nstar == 0 return: nstar < 1 is an argument error; cov's ldc behind the pointers
    "mfgp_gpr_posterior_predict": [({}, WS), (_NS0, ARG), (dict(_NS0, Xs=None, mean=None, var=None), ARG),
                                   ({"ldxs": 3}, ARG), ({"ldm": 1}, ARG), ({"ldc": 0}, WS), ({"cov": J, "ldc": 5}, WS),
                                   ({"cov": J, "ldc": 4}, ARG), ({"cov": J, "ldc": 4, "Xs": None}, ARG), ({"nlf": 2}, WS)],
    "mfgp_gpr_posterior_predict_vjp_workspace_size": [({}, OK), (_NS0, ARG), ({"nlf": 1}, ARG), ({"nlf": 1, "d": 0}, DIM)],
    # nlf != 0 before the nstar == 0 return, that before the geometry and the pointers
    "mfgp_gpr_posterior_predict_vjp": [({}, WS), ({"nlf": 1}, ARG), (dict(_NS0, nlf=1), ARG), (dict(_NS0, n=0), OK),
                                       (dict(_NS0, p=0, ldxs=0), OK), ({"ldxs": 3}, ARG), ({"ldm": 1}, ARG),
                                       ({"ldgx": 3}, ARG), ({"ldgm": 1}, ARG), ({"gmean": None, "ldgm": 0}, WS),
                                       ({"ldgm": 1, "Xs": None}, ARG)],
    # the graph kernel has the value only and its query says so: nlf > 0 is accepted
    "mfgp_gpr_posterior_logdens_workspace_size": [({}, OK), (_NS0, ARG), ({"nlf": 2}, OK)],
    # the nlf range and (nlf && gX) before the nstar == 0 return; the density's geometry with the pointers
    "mfgp_gpr_posterior_logdens": [({}, WS), ({"nlf": 1}, ARG), ({"nlf": 1, "gX": None}, WS), (dict(_NS0, nlf=1), ARG),
                                   (dict(_NS0, nlf=MAX_LF + 1), ARG), (dict(_NS0, nlf=1, gX=None), OK),
                                   (dict(_NS0, n=0), OK), (dict(_NS0, y_rs=-1), OK), ({"y_rs": -1}, ARG), ({"y_rs": 1}, ARG),
                                   ({"y_rs": 0}, WS), ({"ov_rs": 1}, ARG), ({"ov_rs": 0}, WS), ({"ov_rs": -1}, ARG),
                                   ({"obs_cov": J, "ldc": 1}, ARG), ({"obs_cov": J, "ldc": 2}, WS), ({"ldgx": 3}, ARG),
                                   ({"gX": None, "ldgx": 0}, WS), ({"ldxs": 3}, ARG), ({"ldm": 1}, ARG)],
    "mfgp_gpr_posterior_leave_out_workspace_size": [({}, OK), ({"ngroups": 0}, ARG), ({"nrows": 2}, ARG),
                                                    ({"nrows": 3}, OK)],
    # nlf, ngroups < 0 and gmax before the ngroups == 0 return, the rest behind it
    "mfgp_gpr_posterior_leave_out": [({}, WS), ({"ngroups": -1}, ARG), ({"gmax": 0}, ARG), ({"gmax": LO_W + 1}, ARG),
                                     ({"gmax": LO_W, "ldc": LO_W}, WS), ({"ngroups": 0, "gmax": 0}, ARG),
                                     ({"ngroups": 0, "nlf": MAX_LF + 1}, ARG), ({"ngroups": 0, "n": 0}, OK),
                                     ({"ngroups": 0, "nrows": -1, "ldr": 0}, OK), ({"nrows": 2}, ARG), ({"ldr": 1}, ARG),
                                     ({"ldc": 1}, ARG), ({"cov": None, "ldc": 0}, WS)],
    "mfgp_gpr_posterior_design_workspace_size": [({}, OK), ({"qmax": -1}, ARG), ({"qmax": DESIGN_MAXQ + 1}, ARG),
                                                 ({"qmax": DESIGN_MAXQ}, OK), ({"qmax": 0}, OK), ({"nref": -1}, ARG),
                                                 ({"ncand": -1}, ARG), ({"nref": 0}, OK), ({"ncand": 0}, OK),
                                                 ({"nref": 2 ** 30, "ncand": 2 ** 30}, ARG)],
    # geometry and k (<= DESIGN_MAXQ) before the ncand == 0 return; E only with k > 0; nref == 0 sizes as any call
    "mfgp_gpr_posterior_design_score": [({}, WS), ({"k": -1}, ARG), ({"k": DESIGN_MAXQ + 1}, ARG), ({"k": DESIGN_MAXQ}, WS),
                                        ({"ncand": 0, "k": DESIGN_MAXQ + 1}, ARG), ({"ncand": 0, "n": 0}, ARG),
                                        ({"ncand": 0, "nref": -1}, ARG), ({"ncand": 0, "ldx": 0}, OK),
                                        ({"k": 0, "E": None}, WS), ({"k": 0, "ldE": 0}, WS), ({"ldE": 11}, ARG),
                                        ({"ldx": 3}, ARG), ({"nref": 0}, WS), ({"nref": 0, "k": 0, "E": None}, WS),
                                        ({"nref": 0, "score": None}, ARG), ({"refresh": 1, "k": 0}, WS)],
    # k < DESIGN_MAXQ here
    "mfgp_gpr_posterior_design_append": [({}, WS), ({"k": -1}, ARG), ({"k": DESIGN_MAXQ}, ARG), ({"k": DESIGN_MAXQ - 1}, WS),
                                         ({"k": 0}, WS), ({"ncand": 0, "k": DESIGN_MAXQ}, ARG), ({"ncand": 0, "p": 0}, ARG),
                                         ({"ncand": 0, "ldE": 0}, OK), ({"k": 0, "E": None}, ARG), ({"ldE": 11}, ARG),
                                         ({"ldx": 3}, ARG), ({"nref": 0}, WS)],
    "mfgp_gpr_posterior_append_workspace_size": [({}, OK), ({"k": 0}, ARG), ({"k": APPEND_MAXK + 1}, ARG),
                                                 ({"k": APPEND_MAXK}, OK), ({"n": 2 ** 31 - 4096}, ARG)],
    # out_cache == cache is an argument error; Yadd / mean_add optional, their leading dimensions only when given
    "mfgp_gpr_posterior_append": [({}, WS), ({"k": 0}, ARG), ({"k": APPEND_MAXK + 1}, ARG), ({"k": APPEND_MAXK}, WS),
                                  ({"out_cache": J}, ARG), ({"cache": J2}, ARG), ({"ldxa": 3}, ARG), ({"ldya": 1}, ARG),
                                  ({"Yadd": None, "ldya": 0}, WS), ({"ldm": 1}, ARG), ({"mean_add": None, "ldm": 0}, WS),
                                  ({"nlf": 2}, WS)],
    "mfgp_svgp_posterior_size": [({}, OK)],
    # !W && l != p behind the pointers
    "mfgp_svgp_posterior_build": [({}, WS), ({"ldz": 3}, ARG), ({"W": None}, ARG), ({"W": None, "l": 3}, WS),
                                  ({"W": None, "l": 3, "Z": None}, ARG), ({"W": None, "p": 2}, WS)],
    "mfgp_svgp_posterior_predict_workspace_size": [({}, OK), (_NS0, ARG)],
    "mfgp_svgp_posterior_predict": [({}, WS), (_NS0, ARG), (dict(_NS0, Xs=None, f_mu=None, f_var=None), ARG),
                                    ({"ldxs": 3}, ARG), ({"mixed": 0}, ARG), ({"mixed": 0, "l": 3}, WS),
                                    ({"mixed": 0, "l": 3, "Xs": None}, ARG)],
    "mfgp_svgp_posterior_predict_vjp_workspace_size": [({}, OK), (_NS0, ARG)],
    # the nstar == 0 return first behind the handle and d; !mixed && l != p and gmean's ldgm behind the pointers
    "mfgp_svgp_posterior_predict_vjp": [({}, WS), (dict(_NS0, m=0), OK), (dict(_NS0, mixed=0), OK), (dict(_NS0, ldgm=0), OK),
                                        ({"ldxs": 3}, ARG), ({"ldgx": 3}, ARG), ({"mixed": 0}, ARG),
                                        ({"mixed": 0, "l": 3}, WS), ({"ldgm": 2}, ARG), ({"gmean": None, "ldgm": 0}, WS),
                                        ({"ldgm": 2, "gX": None}, ARG)],
    "mfgp_svgp_posterior_logdens_workspace_size": [({}, OK), (_NS0, ARG)],
    "mfgp_svgp_posterior_logdens": [({}, WS), (dict(_NS0, m=0), OK), (dict(_NS0, mixed=0), OK), (dict(_NS0, y_rs=-1), OK),
                                    ({"ldxs": 3}, ARG), ({"mixed": 0}, ARG), ({"mixed": 0, "l": 3}, WS), ({"y_rs": 2}, ARG),
                                    ({"y_rs": 0}, WS), ({"ov_rs": 2}, ARG), ({"ov_rs": -1}, ARG),
                                    ({"obs_cov": J, "ldc": 2}, ARG), ({"obs_cov": J, "ldc": 3}, WS), ({"ldgx": 3}, ARG),
                                    ({"gX": None, "ldgx": 0}, WS)],
}
# the change behind which an entry returns MFGP_OK before it looks at a pointer
POST_EARLY = {"mfgp_gpr_posterior_predict_vjp": _NS0, "mfgp_svgp_posterior_predict_vjp": _NS0,
              "mfgp_gpr_posterior_logdens": _NS0, "mfgp_svgp_posterior_logdens": _NS0,
              "mfgp_gpr_posterior_leave_out": {"ngroups": 0}, "mfgp_gpr_posterior_design_score": {"ncand": 0},
              "mfgp_gpr_posterior_design_append": {"ncand": 0}}


def test_posterior_table_covers_every_entry(lib):
    from multi_fidelity_gpflow_amd._lib import SIGNATURES
    names = {k for k in SIGNATURES if k.startswith(("mfgp_gpr_posterior_", "mfgp_svgp_posterior_"))}
    assert names == set(POST) == set(POST_CASES)
    for k in names:
        assert len(POST[k]) + 1 == len(SIGNATURES[k]), k


@pytest.mark.parametrize("name", sorted(POST_SIZE))
def test_posterior_size_entry_codes(lib, h, name):
    for change, want, handle in _post_common(name):
        assert _call(lib, h, name, change, handle) == want, _show(name, change, handle)
    for change, want in POST_CASES[name] + [({"bytes": None}, ARG)]:
        assert _call(lib, h, name, change) == want, _show(name, change, True)


def _null(change):
    return any(v is None for v in change.values())


@pytest.mark.parametrize("name", sorted(set(POST) - POST_SIZE))
def test_posterior_compute_entry_codes(lib, h, name):
    """The cases that hand over no null pointer beyond the valid call's own optional ones."""
    for change, want, handle in _post_common(name):
        if not _null(change):
            assert _call(lib, h, name, change, handle) == want, _show(name, change, handle)
    for change, want in POST_CASES[name]:
        if not _null(change):
            assert _call(lib, h, name, change) == want, _show(name, change, True)


@pytest.mark.skipif(torch.cuda.is_available(), reason="null-pointer calls are a host-only check")
@pytest.mark.parametrize("name", sorted(set(POST) - POST_SIZE))
def test_posterior_compute_entry_null_pointer_codes(lib, h, name):
    for change, want, handle in _post_common(name):
        if _null(change):
            assert _call(lib, h, name, change, handle) == want, _show(name, change, handle)
    for change, want in POST_CASES[name] + _post_pointers(name, POST_EARLY.get(name)):
        if _null(change):
            assert _call(lib, h, name, change) == want, _show(name, change, True)


def test_setter_and_getter_codes(lib, h):
    """The handle checks of the schedule setters; mfgp_get_step_fusion(NULL) is 0, not MFGP_ERR_ARG."""
    for fn in ("mfgp_set_tiny", "mfgp_set_resident", "mfgp_set_step_fusion", "mfgp_set_flow", "mfgp_set_tile",
               "mfgp_set_f32_panel", "mfgp_set_f32_lookahead", "mfgp_set_f32_reserve", "mfgp_set_f32_refine"):
        assert getattr(lib, fn)(None, 1) == ARG, fn
    assert lib.mfgp_get_step_fusion(None) == 0
    assert lib.mfgp_get_tiny(None) == ARG and lib.mfgp_get_grad_chunk(None) == ARG and lib.mfgp_get_flow(None) == ARG
    assert lib.mfgp_set_f32_panel(h, 65) == ARG and lib.mfgp_set_f32_reserve(h, -1) == ARG
    assert lib.mfgp_set_f32_refine(h, 3) == ARG


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_phase_times_entries_run_the_evaluation(hbs, dtype):
    """mfgp_gpr_lml_phase_times / mfgp_gpr_phase_times_ex (diagnostic timing, otherwise reached only by the
    benchmark and tools/): the marked evaluation is the launch sequence of mfgp_gpr_lml_ex(want_grad = 1), so it
    leaves the same bits in out, and every phase time is a finite non-negative number.  HBS (n = 53): the
    one-launch tiny path and, with it off, the step sequence; fp32: one 128-tile."""
    from multi_fidelity_gpflow_amd.engine import Engine, gpr_phase_times, theta_size
    from multi_fidelity_gpflow_amd._lib import check, ptr
    eng = Engine.get()
    X = torch.tensor(hbs["X"], dtype=dtype, device=eng.device)
    Y = torch.tensor(hbs["Y"], dtype=dtype, device=eng.device)
    n, p, d = X.shape[0], Y.shape[1], X.shape[1] - 1
    th = torch.tensor([1.0] + [1.0] * d + [0.5] + [1.5] * d + [0.9, 1e-2], dtype=torch.float64, device=eng.device)
    ws = eng.private_workspace(eng.gpr_workspace_bytes(n, p, d, dtype))
    info = torch.zeros(1, dtype=torch.int32, device=eng.device)
    k = 8
    try:
        for tiny in ((True, False) if dtype == torch.float64 else (True,)):
            eng.set_tiny(tiny)
            want, _ = eng.gpr_lml(X, Y, th, want_grad=True)
            out = torch.zeros(1 + theta_size(d), dtype=torch.float64, device=eng.device)
            ms, fl, la = (C.c_float * k)(), (C.c_double * k)(), (C.c_int * k)()
            check(eng.lib.mfgp_gpr_phase_times_ex(eng.h, int(dtype == torch.float32), n, p, d, ptr(X), d + 1, ptr(Y), p,
                                                  ptr(th), ptr(ws), ws.numel(), ptr(out), ptr(info), ms, fl, la, k),
                  "mfgp_gpr_phase_times_ex")
            torch.cuda.synchronize()
            assert int(info.item()) == 0
            assert torch.equal(out, want)
            assert all(0.0 <= float(v) < 1e4 for v in ms)
            if dtype == torch.float32:
                assert sum(la) > 0 and sum(fl) > 0.0
            else:
                assert sum(float(v) for v in ms) > 0.0
                direct = gpr_phase_times(eng, X, Y, th)
                assert len(direct) == 5 and all(0.0 <= v < 1e4 for v in direct)
    finally:
        eng.set_tiny(True)
