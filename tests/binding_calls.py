"""The C calls the Python layer makes, recorded without a library, for tests/golden/make_binding_calls.py (run once on the commit
before the binding's marshalling was shared) and tests/test_binding_calls_cpu.py (which replays them).  A helper, not a test module.

`recording()` replaces _hip.lib and _hip.load_library by a stand-in whose olmc_* / ollv_* / olvq_* / oljd_* attributes return 0 and
keep, per call: the symbol; every scalar as the symbol's argtypes convert it (a double as float.hex, an integer as its value, so int(x)
and bool(x) are one argument); every in-pointer by the bytes it points to, the lengths taken from the call itself (dims x bits and dims
words of the Sobol tables, n cells, k options or scenarios, the local-volatility table's fields and doubles, the jump model, the tags);
every out-pointer as null or not, with its length where a ctypes array is passed.  `calls()` drives the wrappers of _hip and the public
methods of the model classes under it and adds what each returned (type, shape, dtype); `refusals()` lists the exception type and message
of the Python layer's refusals, one fault and two faults at a time; `packed_calls()` and `packed_refusals()` give both the form the
fixtures keep (symbols and a digest per driver; each message once).  Nothing here is an oracle: both compare a tree with its parent.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import hashlib
import itertools
import json
import warnings

import numpy as np

import optionslab_amd as ol
from optionslab_amd import _hip
from optionslab_amd import heston as hes
from tests import call_catalogue as cc
from tests import path_kernels_calls as pk

_D, _U32P, _DP, _I32P = C.c_double, C.POINTER(C.c_uint32), C.POINTER(C.c_double), C.POINTER(C.c_int32)
_COUNTED = {C.POINTER(_hip.Option): _hip.Option, C.POINTER(_hip.HestonScenario): _hip.HestonScenario}      # in-arrays: count = the next scalar
_COUNTED_FIRST = {"olmc_combine_cv": _hip.CvMoments, "olmc_combine_stats": _hip.Stats}                      # argument 0 is an in-array there
_POINTERS = (C._Pointer, C.Array, type(C.byref(C.c_int())))


def prototypes():
    return {**_hip.PROTOTYPES, **_hip.LV_PROTOTYPES, **_hip.LVQ_PROTOTYPES, **_hip.JD_PROTOTYPES}


def _is_pointer_type(t) -> bool:
    return isinstance(t, type) and issubclass(t, C._Pointer)


def _address(arg):
    """The address a pointer argument carries (a POINTER instance, a ctypes array or struct, or byref of one)."""
    if hasattr(arg, "_obj"):                    # byref(x)
        return C.addressof(arg._obj)
    if isinstance(arg, C._Pointer):
        return C.cast(arg, C.c_void_p).value
    return C.addressof(arg)


def _digest(arg, nbytes: int):
    return dict(bytes=int(nbytes), sha256=hashlib.sha256(C.string_at(_address(arg), int(nbytes))).hexdigest())


def _scalar(t, v):
    if t is _D:
        return float(t(v).value).hex()
    if t is C.c_void_p:
        return v.value if isinstance(v, C.c_void_p) else v
    return t(v).value


def _out(arg):
    if arg is None:
        return "null"
    return f"out[{len(arg)}]" if isinstance(arg, C.Array) else "out"


def _record(symbol: str, argtypes, args):
    if len(args) != len(argtypes):
        raise TypeError(f"{symbol} takes {len(argtypes)} arguments, got {len(args)}")
    rec, i = [], 0
    scalars = [None if _is_pointer_type(t) else j for j, t in enumerate(argtypes)]
    for i, (t, a) in enumerate(zip(argtypes, args)):
        if not _is_pointer_type(t):
            rec.append(_scalar(t, a))
            continue
        if a is not None and not isinstance(a, _POINTERS):
            raise TypeError(f"{symbol} argument {i}: {type(a).__name__} is no pointer")
        following = next((args[j] for j in scalars[i + 1:] if j is not None), None)
        if t is _U32P and i + 2 < len(argtypes) and argtypes[i + 1] is _U32P and argtypes[i + 2] is C.c_int32:          # the Sobol run
            dims = int(args[i - 1]) * (2 if "heston" in symbol else 1)
            rec.append(dict(sv=_digest(a, 4 * dims * int(args[i + 2]))))
        elif t is _U32P and i >= 1 and argtypes[i - 1] is _U32P and i + 1 < len(argtypes) and argtypes[i + 1] is C.c_int32:
            dims = int(args[i - 2]) * (2 if "heston" in symbol else 1)
            rec.append(dict(shift=_digest(a, 4 * dims)))
        elif t is _U32P and symbol == "olmc_european_multi":
            rec.append("null" if a is None else dict(tags=_digest(a, 4 * int(following))))
        elif t in _COUNTED:
            rec.append(dict(array=_digest(a, C.sizeof(_COUNTED[t]) * int(following))))
        elif i == 0 and symbol in _COUNTED_FIRST:
            rec.append(dict(array=_digest(a, C.sizeof(_COUNTED_FIRST[symbol]) * int(following))))
        elif t is _DP and i + 2 < len(argtypes) and argtypes[i + 1] is _I32P and argtypes[i + 2] is C.c_int32:          # the cells' strikes
            rec.append(dict(strikes=_digest(a, 8 * int(args[i + 2]))))
        elif t is _I32P and i >= 1 and argtypes[i - 1] is _DP and i + 1 < len(argtypes) and argtypes[i + 1] is C.c_int32:
            rec.append(dict(steps=_digest(a, 4 * int(args[i + 1]))))
        elif t is C.POINTER(_hip.LvSurface):
            s = a._obj if hasattr(a, "_obj") else a.contents
            rec.append(dict(lv=[s.n_x, s.n_t, s.x_lo.hex(), s.x_hi.hex(), s.t_hi.hex()], vol=_digest(s.vol, 8 * s.n_x * s.n_t)))
        elif t is C.POINTER(_hip.JdModel):
            rec.append(dict(model=_digest(a, C.sizeof(_hip.JdModel))))
        else:
            rec.append(_out(a))
    return [symbol] + rec


class Recorder:
    """Stands where the loaded library stands: every prototype is an attribute that records its call and returns 0."""

    def __init__(self):
        self.log = []
        self.asked = 0          # how often _hip.lib() or _hip.load_library() was asked for the library
        for symbol, (_res, argtypes) in prototypes().items():
            setattr(self, symbol, self._entry(symbol, argtypes))

    def _entry(self, symbol, argtypes):
        def call(*args):
            self.log.append(_record(symbol, argtypes, args))
            return 0
        return call

    def take(self):
        log, self.log, self.asked = self.log, [], 0
        return log


@contextlib.contextmanager
def recording():
    rec = Recorder()
    saved = _hip.lib, _hip.load_library

    def library():
        rec.asked += 1
        return rec
    _hip.lib = _hip.load_library = library
    try:
        yield rec
    finally:
        _hip.lib, _hip.load_library = saved


def describe(x):
    """Type, shape and dtype of what a wrapper returned."""
    if isinstance(x, np.ndarray):
        return ["ndarray", list(x.shape), str(x.dtype)]
    if isinstance(x, (list, tuple)):
        items = [describe(y) for y in x]
        if len(items) > 2 and all(item == items[0] for item in items):
            items = [f"{len(items)} x", items[0]]
        return [type(x).__name__, items]
    if isinstance(x, dict):
        return [type(x).__name__, [[k, describe(v)] for k, v in x.items()]]
    return type(x).__name__


# ---------------------------------------------------------------------------------------------------- the calls ----
N, n = 257, 13
S, K, T, R, Q, SIGMA = 100.0, 105.0, 1.0, 0.05, 0.01, 0.2
SEED = 20240229
STRIKES, MATURITIES = (95.0, 100.0, 110.0), (2 / 12, 4 / 12, 6 / 12, 8 / 12, 10 / 12, 1.0)      # 18 cells on 12 steps: two launches
JD = (False, 0.5, -0.1, 0.2, 0.0)


def _heston():
    return ol.HestonPricer(*cc.HESTON)


def _dupire():
    model = ol.DupireLocalVol(R, Q, n_paths=N, n_steps=n, seed=SEED)
    from optionslab_amd.local_vol import create_sample_iv_surface

    strikes, expiries, ivs = create_sample_iv_surface(100.0, 8, 5)
    model.calibrate(strikes, expiries, ivs, 100.0)
    return model


def _direct():
    h = _hip
    opts = [(100.0 + i, 100.0, 1.0, 0.05, 0.2, 0.0, i % 2 == 0) for i in range(3)]
    return {
        "jd_autocallable": lambda: h.jd_autocallable(S, T, R, SIGMA, Q, JD, *cc.AUTOCALL, 4, N, n, SEED, True, 5),
        "jd_cliquet": lambda: h.jd_cliquet(S, T, R, SIGMA, Q, cc.KOU, *cc.CLIQUET, 4, N, n, SEED),
        "fetch_dev-null-stream": lambda: h.fetch_dev(4096, 3),
        "heston_scenario_layout": lambda: h.heston_scenario_layout(cc._scenario_set()),
        "contract_layout": lambda: h.contract_layout(opts, n),
        "combine_stats": lambda: h.combine_stats([(1.0, 2.0, 3), (4.0, 5.0, 6)], R, T),
        "combine_cv": lambda: h.combine_cv([h.CvMoments(1.0, 2.0, 3.0, 4.0, 5.0, 6, 0.0)], S, T, R, Q),
        "european_greeks_fd-evals": lambda: h.european_greeks_fd(S, K, T, R, SIGMA, Q, True, N, n, SEED, True),
    }


def _methods():
    """{label: callable} over the public pricing and simulation methods, fixed seeds, at most 257 paths x 13 steps."""
    out = {}
    hp = _heston()
    for method, pc, scheme in itertools.product(("pseudo", "qmc"), ("bridge", "sequential"), ("euler", "qe")):
        if scheme == "qe" and method == "qmc" and pc == "bridge":
            continue
        tag = f"heston-{method}-{pc}-{scheme}"
        kw = dict(method=method, path_construction=pc)
        kws = dict(kw, scheme=scheme)
        for anti in (False, True):
            out[f"{tag}-price_monte_carlo-anti{int(anti)}"] = lambda kws=kws, anti=anti: hp.price_monte_carlo(S, K, T, R, Q, "put", N, n, SEED, anti, True, **kws)
        out[f"{tag}-price_surface"] = lambda kws=kws: hp.price_surface(S, STRIKES, MATURITIES, R, Q, "call", N, 12, SEED, True, True, **kws)
        out[f"{tag}-simulate_paths"] = lambda kws=kws: hp.simulate_paths(S, T, R, Q, N, n, SEED, **kws)
        out[f"{tag}-price_autocallable"] = lambda kws=kws: hp.price_autocallable(S, T, R, Q, *cc.AUTOCALL, 4, N, n, SEED, True, **kws)
        out[f"{tag}-price_autocallable-no-date"] = lambda kws=kws: hp.price_autocallable(S, T, R, Q, observation_freq=21, n_paths=N, n_steps=n, seed=SEED, **kws)
        out[f"{tag}-price_cliquet"] = lambda kws=kws: hp.price_cliquet(S, T, R, Q, *cc.CLIQUET, 4, N, n, SEED, False, True, **kws)
        if scheme == "qe":
            continue
        out[f"{tag}-price_scenarios"] = lambda kw=kw: hp.price_scenarios(
            [dict(S=S, K=K, T=T, r=R), dict(S=S, K=K, T=0.5, r=R, q=Q, option_type="put", rho=-0.2)] + [dict(S=S + i, K=K, T=T, r=R, v0=0.04 + 0.01 * (i % 7)) for i in range(17)],
            N, n, SEED, True, True, **kw)
        for avg in ("arithmetic", "geometric"):
            out[f"{tag}-price_asian-{avg}"] = lambda kw=kw, avg=avg: hp.price_asian(S, K, T, R, Q, "call", avg, N, n, SEED, True, True, **kw)
        for kind in _hip.BARRIER_KINDS:
            out[f"{tag}-price_barrier-{kind}"] = lambda kw=kw, kind=kind: hp.price_barrier(S, K, T, R, 112.0 if kind[0] == "u" else 90.0, Q, "put", kind, N, n, SEED, **kw)
        out[f"{tag}-price_barrier-odd-name"] = lambda kw=kw: hp.price_barrier(S, K, T, R, 112.0, barrier_type="upward-knock", n_paths=N, n_steps=n, seed=SEED, **kw)
        for lb in ("floating", "fixed"):
            out[f"{tag}-price_lookback-{lb}"] = lambda kw=kw, lb=lb: hp.price_lookback(S, K, T, R, Q, "call", lb, N, n, SEED, False, True, **kw)
        for second in (False, True):
            out[f"{tag}-fused_greeks-{int(second)}"] = lambda kw=kw, second=second: hes.HestonMCAdapter(hp, N, n, SEED, True, **kw)._fused_greeks(
                S, K, T, R, SIGMA, "call", Q, second)
        out[f"{tag}-adapter-price"] = lambda kw=kw: hes.HestonMCAdapter(hp, N, n, SEED, False, **kw).price(S, K, T, R, SIGMA, "put", Q)

    for tag, make in (("dupire", _dupire), ("dupire-qmc-bridge", lambda: _dupire().qmc()), ("dupire-qmc-sequential", lambda: _dupire().qmc("sequential")),
                      ("dupire-flat", lambda: ol.DupireLocalVol(R, Q, n_paths=N, n_steps=n, seed=SEED))):
        out[f"{tag}-price_monte_carlo"] = lambda make=make: make().price_monte_carlo(S, K, T, R, Q, "put", antithetic=True, return_error=True)
        out[f"{tag}-price_monte_carlo-sizes"] = lambda make=make: make().price_monte_carlo(S, K, T, R, Q, "call", 100, 5, 7)
        out[f"{tag}-price"] = lambda make=make: make().price(S, K, T, R, SIGMA, "call", Q)
        out[f"{tag}-simulate_paths"] = lambda make=make: make().simulate_paths(S, T, R, Q, 100, 5, 3)
        for avg in ("arithmetic", "geometric"):
            out[f"{tag}-price_asian-{avg}"] = lambda make=make, avg=avg: make().price_asian(S, K, T, R, Q, "call", avg, antithetic=True)
        for kind in _hip.BARRIER_KINDS:
            out[f"{tag}-price_barrier-{kind}"] = lambda make=make, kind=kind: make().price_barrier(S, K, T, R, 112.0 if kind[0] == "u" else 90.0, Q, "call", kind, return_error=True)
        for lb in ("floating", "fixed"):
            out[f"{tag}-price_lookback-{lb}"] = lambda make=make, lb=lb: make().price_lookback(S, K, T, R, Q, "put", lb)
        out[f"{tag}-price_surface"] = lambda make=make: make().price_surface(S, STRIKES, MATURITIES, R, Q, "call", N, 12, SEED, True, True)

    for tag, model in (("merton", ol.MertonJumpDiffusion(0.5, -0.1, 0.2)), ("kou", ol.KouJumpDiffusion(1.0, 0.4, 10.0, 5.0))):
        for flag in (False, True):
            out[f"{tag}-price_monte_carlo-anti{int(flag)}"] = lambda model=model, flag=flag: model.price_monte_carlo(S, K, T, R, SIGMA, "put", Q, N, n, SEED, True, antithetic=flag)
            out[f"{tag}-simulate_paths-mirror{int(flag)}"] = lambda model=model, flag=flag: model.simulate_paths(S, T, R, SIGMA, Q, N, n, SEED, mirror=flag)
            out[f"{tag}-price_asian-anti{int(flag)}"] = lambda model=model, flag=flag: model.price_asian(S, K, T, R, SIGMA, Q, "call", "geometric" if flag else "arithmetic", N, n, SEED, flag)
            out[f"{tag}-price_lookback-anti{int(flag)}"] = lambda model=model, flag=flag: model.price_lookback(S, K, T, R, SIGMA, Q, "call", "fixed" if flag else "floating", N, n, SEED, flag, True)
            out[f"{tag}-price_surface-anti{int(flag)}"] = lambda model=model, flag=flag: model.price_surface(S, STRIKES, MATURITIES, R, SIGMA, Q, "put", N, 12, SEED, flag, flag)
            out[f"{tag}-price_autocallable-anti{int(flag)}"] = lambda model=model, flag=flag: model.price_autocallable(S, T, R, SIGMA, Q, *cc.AUTOCALL, 21 if flag else 4, N, n, SEED, flag)
            out[f"{tag}-price_cliquet-anti{int(flag)}"] = lambda model=model, flag=flag: model.price_cliquet(S, T, R, SIGMA, Q, *cc.CLIQUET, 4, N, n, SEED, flag, True)
        for kind in _hip.BARRIER_KINDS:
            out[f"{tag}-price_barrier-{kind}"] = lambda model=model, kind=kind: model.price_barrier(S, K, T, R, SIGMA, 112.0 if kind[0] == "u" else 90.0, Q, "call", kind, N, n, SEED, True)
    out["merton-simulate_path"] = lambda: ol.MertonJumpDiffusion(0.5, -0.1, 0.2).simulate_path(S, T, R, SIGMA, Q, n, SEED)

    from optionslab_amd import exotic as ex

    spot = dict(S=S, K=K, T=T, r=R, sigma=SIGMA, q=Q, seed=SEED)
    for method, pc in (("pseudo", "bridge"), ("qmc", "bridge"), ("qmc", "sequential")):
        kw = dict(method=method, path_construction=pc)
        tag = f"exotic-{method}-{pc}"
        for avg in ("arithmetic", "geometric"):
            out[f"{tag}-asian-{avg}"] = lambda kw=kw, avg=avg: ex.AsianOption(**spot).price(N, n, avg, "call", True, True, **kw)
        if method == "pseudo":
            out[f"{tag}-asian-fp32"] = lambda kw=kw: ex.AsianOption(**spot).price(N, n, precision="fp32", **kw)
        for kind in _hip.BARRIER_KINDS:
            out[f"{tag}-barrier-{kind}"] = lambda kw=kw, kind=kind: ex.BarrierOption(**spot, barrier=112.0 if kind[0] == "u" else 90.0).price(N, n, kind, "put", False, True, **kw)
        out[f"{tag}-barrier-at-spot"] = lambda kw=kw: ex.BarrierOption(**dict(spot, S=100.0), barrier=100.0).price(N, n, **kw)
        for lb in ("floating", "fixed"):
            out[f"{tag}-lookback-{lb}"] = lambda kw=kw, lb=lb: ex.LookbackOption(**spot).price(N, n, lb, "call", True, **kw)
        out[f"{tag}-american"] = lambda kw=kw: ex.AmericanOption(**spot).price(N, n, "put", 3, True, **kw)
        out[f"{tag}-american-boundary"] = lambda kw=kw: ex.AmericanOption(**spot).early_exercise_boundary(N, n, "call", **kw)
        out[f"{tag}-autocallable"] = lambda kw=kw: ex.AutocallableOption(**spot).price(N, n, 4, True, True, **kw)
        out[f"{tag}-autocallable-no-date"] = lambda kw=kw: ex.AutocallableOption(**spot).price(N, n, 21, option_type="call", **kw)
        out[f"{tag}-cliquet"] = lambda kw=kw: ex.CliquetOption(**spot).price(N, n, 4, False, True, **kw)
    out["exotic-price_barrier"] = lambda: ex.price_barrier(S, K, T, R, SIGMA, 112.0, n_paths=N, seed=SEED)
    out["exotic-price_asian"] = lambda: ex.price_asian(S, K, T, R, SIGMA, "geometric", "put", N, SEED)
    out["exotic-price_american"] = lambda: ex.price_american(S, K, T, R, SIGMA, "put", N, SEED)

    from optionslab_amd import simulation as sim

    out["simulation-paths"] = lambda: sim.simulate_gbm_paths_hip(S, T, R, SIGMA, Q, N, n, SEED)
    out["simulation-qmc-paths"] = lambda: sim.simulate_gbm_qmc_paths_hip(S, T, R, SIGMA, Q, N, n, SEED, "sequential")
    out["simulation-qmc-antithetic"] = lambda: sim.simulate_gbm_qmc_antithetic_hip(S, T, R, SIGMA, Q, N, n, SEED)
    for method in (ol.MCMethod.HIP, ol.MCMethod.QMC):
        for gpus in (1, 2):
            mc = lambda method=method, gpus=gpus: ol.MonteCarloPricer(N, n, SEED, method, n_gpus=gpus)      # noqa: E731
            tag = f"mc-{method.value}-gpus{gpus}"
            out[f"{tag}-price"] = lambda mc=mc: mc().price(S, K, T, R, SIGMA, "call", Q, return_error=True)
            out[f"{tag}-cv"] = lambda mc=mc: mc().price_with_control_variate(S, K, T, R, SIGMA, "put", Q)
            out[f"{tag}-greeks"] = lambda mc=mc: mc().greeks(S, K, T, R, SIGMA, "call", Q)
    uni = lambda: ol.MonteCarloPricerUni(N, n, SEED)      # noqa: E731
    out["uni-price"] = lambda: uni().price(S, K, T, R, SIGMA, "call", Q)
    out["uni-delta_gamma"] = lambda: uni().delta_gamma(S, K, T, R, SIGMA, "put", Q, seed=5)
    out["uni-delta_gamma_batch"] = lambda: uni().delta_gamma_batch([S, S + 1], [K, K], [T, T], [R, R], [SIGMA, SIGMA], "call", Q)
    return out


def drivers():
    """{label: zero-argument callable}: the catalogue without its caller_stream entries, every group of the path kernels' calls, the
    direct calls and the public methods."""
    out = {f"catalogue/{e.name}": e.call for e in cc.catalogue() if "caller_stream" not in e.state}
    for group in pk.GROUPS:
        out.update({f"path-kernels/{group}/{label}": call for label, call in pk.calls(group, N, n).items()})
    out.update({f"direct/{label}": call for label, call in _direct().items()})
    out.update({f"method/{label}": call for label, call in _methods().items()})
    return out


def calls():
    """{label: {"calls": [...], "returns": ...}} of every driver under the recording stand-in."""
    doc = {}
    with recording() as rec, warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for label, call in drivers().items():
            result = call()
            doc[label] = dict(calls=rec.take(), returns=describe(result))
    return doc


# ------------------------------------------------------------------------------------------------ the refusals ----
COUNTS = {"n_paths=0": dict(n_paths=0), "n_steps=0": dict(n_steps=0)}
QMC = {"method=x": dict(method="sobol"), "path_construction=x": dict(path_construction="zigzag"),
       "qmc-too-many-paths": dict(method="qmc", n_paths=(1 << 30) + 1), "qmc-bridge-too-many-steps": dict(method="qmc", n_steps=1025)}
SCHEME = {"scheme=x": dict(scheme="milstein"), "qe-on-bridge": dict(scheme="qe", method="qmc")}
SURFACE = {"no-strikes": dict(strikes=[]), "no-maturities": dict(maturities=[]), "maturity<=0": dict(maturities=[0.5, 0.0]),
           "maturity-nan": dict(maturities=[float("nan")]), "maturity-off-grid": dict(maturities=[1.0, 0.3], n_steps=4)}
ASIAN, BARRIER, LOOKBACK = ({"avg_type=x": dict(avg_type="harmonic")}, {"barrier=0": dict(barrier=0.0), "barrier_type=7": dict(barrier_type=7)},
                           {"lookback_type=x": dict(lookback_type="partial")})
AUTOCALL, CLIQUET = {"observation_freq=0": dict(observation_freq=0)}, {"n_periods=0": dict(n_periods=0), "n_periods>n_steps": dict(n_periods=14, n_steps=13)}
SCENARIOS = {"no-scenarios": dict(scenarios=[]), "scenario-lacks-key": dict(scenarios=[dict(S=S, K=K, r=R)]),
             "scenario-unknown-key": dict(scenarios=[dict(S=S, K=K, T=T, r=R, vol=0.2)]), "scenario-T<=0": dict(scenarios=[dict(S=S, K=K, T=0.0, r=R)]),
             "scenario-rho": dict(scenarios=[dict(S=S, K=K, T=T, r=R, rho=1.5)]), "euler-only": dict(scheme="qe")}


def _refusal_cases():
    """(label, callable(**kwargs), base kwargs, {fault: overriding kwargs}) per public method."""
    hp = _heston()
    contract = dict(S=S, K=K, T=T, r=R)
    sizes = dict(n_paths=N, n_steps=n, seed=SEED)
    surface = dict(S=S, strikes=list(STRIKES), maturities=[0.5, 1.0], r=R, n_paths=N, n_steps=12, seed=SEED)
    cases = [
        ("heston.price_monte_carlo", hp.price_monte_carlo, {**contract, **sizes}, {**COUNTS, **QMC, **SCHEME}),
        ("heston.price_surface", hp.price_surface, surface, {**COUNTS, **QMC, **SCHEME, **SURFACE}),
        ("heston.price_scenarios", hp.price_scenarios, dict(scenarios=[contract], **sizes), {**COUNTS, **QMC, "scheme=x": SCHEME["scheme=x"], **SCENARIOS}),
        ("heston.simulate_paths", hp.simulate_paths, dict(S=S, T=T, r=R, **sizes), {**COUNTS, **QMC, **SCHEME}),
        ("heston.price_asian", hp.price_asian, {**contract, **sizes}, {**COUNTS, **QMC, **ASIAN}),
        ("heston.price_barrier", hp.price_barrier, dict(contract, barrier=120.0, **sizes), {**COUNTS, **QMC, **BARRIER}),
        ("heston.price_lookback", hp.price_lookback, {**contract, **sizes}, {**COUNTS, **QMC, **LOOKBACK}),
        ("heston.price_autocallable", hp.price_autocallable, dict(S=S, T=T, r=R, **sizes), {**COUNTS, **QMC, **SCHEME, **AUTOCALL}),
        ("heston.price_cliquet", hp.price_cliquet, dict(S=S, T=T, r=R, **sizes), {**COUNTS, **QMC, **SCHEME, **CLIQUET}),
        ("heston.HestonMCAdapter", lambda **kw: hes.HestonMCAdapter(hp, **kw), sizes, {**COUNTS, **QMC, "scheme=x": SCHEME["scheme=x"], "euler-only": dict(scheme="qe")}),
    ]
    for tag, make in (("dupire", _dupire), ("dupire.qmc", lambda: _dupire().qmc())):
        m = make()
        qmc = {"qmc-too-many-paths": dict(n_paths=(1 << 30) + 1), "qmc-bridge-too-many-steps": dict(n_steps=1025)} if tag == "dupire.qmc" else {}
        cases += [
            (f"{tag}.price_monte_carlo", m.price_monte_carlo, contract, {**COUNTS, **qmc}),
            (f"{tag}.simulate_paths", m.simulate_paths, dict(S=S, T=T, r=R, n_paths=N, n_steps=n, seed=SEED), {**COUNTS, **qmc}),
            (f"{tag}.price_asian", m.price_asian, contract, {**COUNTS, **qmc, **ASIAN}),
            (f"{tag}.price_barrier", m.price_barrier, dict(contract, barrier=120.0), {**COUNTS, **qmc, **BARRIER}),
            (f"{tag}.price_lookback", m.price_lookback, contract, {**COUNTS, **qmc, **LOOKBACK}),
            (f"{tag}.price_surface", m.price_surface, dict(surface), {**COUNTS, **qmc, **SURFACE}),
        ]
    cases.append(("dupire.qmc-view", lambda **kw: _dupire().qmc(**kw), {}, {"path_construction=x": dict(path_construction="zigzag")}))
    cases.append(("dupire.local_vol_table", lambda **kw: _dupire().local_vol_table(S, T, **kw), {}, {"n_x=1": dict(n_x=1), "n_t=0": dict(n_t=0)}))
    for tag, m in (("merton", ol.MertonJumpDiffusion(0.5, -0.1, 0.2)), ("kou", ol.KouJumpDiffusion(1.0, 0.4, 10.0, 5.0))):
        jc = dict(contract, sigma=SIGMA)
        cases += [
            (f"{tag}.price_monte_carlo", m.price_monte_carlo, {**jc, **sizes}, {**COUNTS, "n_paths=0-antithetic": dict(n_paths=0, antithetic=True)}),
            (f"{tag}.simulate_paths", m.simulate_paths, dict(S=S, T=T, r=R, sigma=SIGMA, **sizes), {**COUNTS, "n_steps=0-mirror": dict(n_steps=0, mirror=True)}),
            (f"{tag}.price_asian", m.price_asian, {**jc, **sizes}, {**COUNTS, **ASIAN}),
            (f"{tag}.price_barrier", m.price_barrier, dict(jc, barrier=120.0, **sizes), {**COUNTS, **BARRIER}),
            (f"{tag}.price_lookback", m.price_lookback, {**jc, **sizes}, {**COUNTS, **LOOKBACK}),
            (f"{tag}.price_surface", m.price_surface, dict(surface, sigma=SIGMA), {**COUNTS, **SURFACE}),
            (f"{tag}.price_autocallable", m.price_autocallable, dict(S=S, T=T, r=R, sigma=SIGMA, **sizes), {**COUNTS, **AUTOCALL}),
            (f"{tag}.price_cliquet", m.price_cliquet, dict(S=S, T=T, r=R, sigma=SIGMA, **sizes), {**COUNTS, **CLIQUET}),
        ]
    from optionslab_amd import exotic as ex
    from optionslab_amd import simulation as sim

    spot = dict(S=S, K=K, T=T, r=R, sigma=SIGMA, q=Q, seed=SEED)
    qmc_steps = {"qmc-too-many-steps": dict(method="qmc", path_construction="sequential", n_steps=21202)}
    run = dict(n_paths=N, n_steps=n)
    cases += [
        ("exotic.AsianOption.price", ex.AsianOption(**spot).price, run,
         {**COUNTS, **QMC, **qmc_steps, "precision=x": dict(precision="fp16"), "qmc-fp32": dict(method="qmc", precision="fp32")}),
        ("exotic.BarrierOption.price", ex.BarrierOption(**spot, barrier=120.0).price, run, {**COUNTS, **QMC, **qmc_steps, "barrier_type=7": dict(barrier_type=7)}),
        ("exotic.BarrierOption.price-no-barrier", ex.BarrierOption(**spot).price, run, {"as-it-is": {}, **COUNTS, **QMC, "barrier_type=7": dict(barrier_type=7)}),
        ("exotic.LookbackOption.price", ex.LookbackOption(**spot).price, run, {**COUNTS, **QMC, **qmc_steps}),
        ("exotic.AmericanOption.price", ex.AmericanOption(**spot).price, run, {**COUNTS, **QMC, **qmc_steps}),
        ("exotic.AmericanOption.early_exercise_boundary", ex.AmericanOption(**spot).early_exercise_boundary, run, {**COUNTS, **QMC, **qmc_steps}),
        ("exotic.AutocallableOption.price", ex.AutocallableOption(**spot).price, run, {**COUNTS, **QMC, **qmc_steps}),
        ("exotic.CliquetOption.price", ex.CliquetOption(**spot).price, run, {**COUNTS, **QMC, **qmc_steps}),
        ("simulation.simulate_gbm_paths_hip", sim.simulate_gbm_paths_hip, dict(S=S, T=T, r=R, sigma=SIGMA, q=Q, seed=SEED, **run), COUNTS),
        ("simulation.simulate_gbm_qmc_paths_hip", sim.simulate_gbm_qmc_paths_hip, dict(S=S, T=T, r=R, sigma=SIGMA, q=Q, seed=SEED, **run),
         {**COUNTS, "path_construction=x": QMC["path_construction=x"], "qmc-bridge-too-many-steps": dict(n_steps=1025)}),
        ("simulation.simulate_gbm_hip", sim.simulate_gbm_hip, dict(S=S, T=T, r=R, sigma=SIGMA, q=Q, seed=SEED, **run), COUNTS),
        ("heston.calibration_objective", lambda **kw: hes.calibration_objective(
            dict(spot=S, strikes=kw.pop("strikes", list(STRIKES)), maturities=kw.pop("maturities", [0.5, 1.0]), market_ivs=kw.pop("market_ivs", np.full((3, 2), 0.2)), r=R), **kw),
         dict(n_paths=N, n_steps=12), {"n_paths=0": dict(n_paths=0), **QMC, **SCHEME, **SURFACE, "seed=None": dict(seed=None), "ivs-shape": dict(market_ivs=np.zeros((2, 2)))}),
    ]
    return cases


def _sobol_wrapper_refusals():
    """_hip's own refusals: a point range beyond the tables' columns, an odd number of Heston dimensions, ragged cells, a bad table."""
    from optionslab_amd.monte_carlo import SobolDirections

    sv, shift = cc.tables(13, cc.SEED_A)
    short = SobolDirections(np.ascontiguousarray(sv), 8)
    euro = (S, K, T, R, SIGMA, Q)
    return {
        "european_qmc-beyond-valid-bits": lambda: _hip.european_qmc(*euro, True, 257, short, shift),
        "european_qmc-offset-beyond-valid-bits": lambda: _hip.european_qmc(*euro, True, 100, short, shift, point_offset=200),
        "asian_qmc-beyond-30-bits": lambda: _hip.asian_qmc(*euro, True, False, (1 << 30) + 1, sv, shift),
        "heston_qmc-odd-dimensions": lambda: _hip.heston_qmc(S, K, T, R, Q, True, *cc.HESTON, 257, sv, shift),
        "heston_qmc-beyond-and-odd": lambda: _hip.heston_qmc(S, K, T, R, Q, True, *cc.HESTON, 257, short, shift),
        "heston_qmc_paths-odd-dimensions": lambda: _hip.heston_qmc_paths(S, T, R, Q, *cc.HESTON, 257, sv, shift),
        "heston_qmc_surface-odd-and-ragged": lambda: _hip.heston_qmc_surface(S, T, R, Q, True, *cc.HESTON, [100.0], [1, 2], 257, sv, shift),
        "heston_qmc_scenarios-odd-dimensions": lambda: _hip.heston_qmc_scenarios(cc._scenario_set(), 257, sv, shift),
        "heston_qmc_greeks_fd-odd-dimensions": lambda: _hip.heston_qmc_greeks_fd(*euro, True, *cc.HESTON[:4], 257, sv, shift, True, False, True),
        "heston_autocallable_qmc-odd-dimensions": lambda: _hip.heston_autocallable_qmc(S, T, R, Q, *cc.HESTON, *cc.AUTOCALL, 4, 257, sv, shift),
        "heston_surface-ragged-cells": lambda: _hip.heston_surface(S, T, R, Q, True, *cc.HESTON, [100.0, 105.0], [1], 257, 13, SEED),
        "lvq_surface_prices-beyond-and-ragged": lambda: _hip.lvq_surface_prices(S, T, R, Q, True, pk.TABLE_ARGS, [100.0], [1, 2], 257, short, shift),
        "lv_price-bad-table": lambda: _hip.lv_price(S, K, T, R, Q, True, (np.zeros((2, 2, 2)), -1.0, 1.0, 1.0), 8, 0.0, 257, 13, SEED),
        "lvq_price-beyond-and-bad-table": lambda: _hip.lvq_price(S, K, T, R, Q, True, (np.zeros((2, 2, 2)), -1.0, 1.0, 1.0), 8, 0.0, 257, short, shift),
    }


def refusals():
    """{label: [exception type, message]} -- "none" where a call is not refused: every fault alone and every pair of faults whose
    keyword arguments do not collide, per public method; under the recording stand-in.  A refusal must come before the library is so
    much as asked for (_hip.lib(), _hip.load_library()), let alone called: one that does not gets a third entry that says so, which no
    fixture holds."""
    doc = {}

    def attempt(label, call, **kwargs):
        rec.take()
        try:
            call(**kwargs)
        except Exception as e:      # noqa: BLE001 -- the type is what is recorded
            doc[label] = [type(e).__name__, str(e)]
            if rec.asked or rec.log:
                doc[label].append(f"AFTER the library was asked for {rec.asked} time(s) and called {len(rec.log)} time(s)")
        else:
            doc[label] = "none"

    with recording() as rec, warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for label, call, base, faults in _refusal_cases():
            for name, kw in faults.items():
                attempt(f"{label}/{name}", call, **{**base, **kw})
            for (a, kwa), (b, kwb) in itertools.combinations(faults.items(), 2):
                if any(key in kwb and kwb[key] is not kwa[key] and kwb[key] != kwa[key] for key in kwa):
                    continue
                attempt(f"{label}/{a}+{b}", call, **{**base, **kwa, **kwb})
        for label, call in _sobol_wrapper_refusals().items():
            attempt(f"_hip/{label}", call)
        rec.take()              # the calls of what was not refused are tests/golden/binding_calls.json's business
    return doc


# ------------------------------------------------------------------------------------------------ the fixtures' form ----
def packed_calls(doc):
    """{group: {label: "symbol+symbol ... digest"}}: per driver the symbols it reached, in order, and the first 32 hex digits of the
    sha256 of its whole record as canonical JSON -- equal digests are equal records (every scalar, digest of bytes, out-pointer and
    return shape).  The group is the label up to its second word; a group is one line of the fixture."""
    out = {}
    for label, rec in doc.items():
        text = json.dumps(rec, sort_keys=True, separators=(",", ":"))
        head, _, rest = label.partition("/")
        group = head + "/" + rest.replace("/", "-").split("-")[0]
        out.setdefault(group, {})[label] = "+".join(call[0] for call in rec["calls"]) + " " + hashlib.sha256(text.encode()).hexdigest()[:32]
    return out


def packed_refusals(doc):
    """{"messages": [[type, message], ...], "cases": {method: {faults: index into messages, -1 = not refused}}}."""
    messages, cases = [], {}
    for label, got in doc.items():
        case, _, faults = label.partition("/")
        if got != "none" and list(got) not in messages:
            messages.append(list(got))
        cases.setdefault(case, {})[faults] = -1 if got == "none" else messages.index(list(got))
    return dict(messages=messages, cases=cases)


def dump_lines(doc, f, keys=()):
    """JSON with one line per entry of the top-level mapping (and of the mappings named in `keys`)."""
    def entries(d, depth):
        return ",\n".join(" " * depth + json.dumps(k) + ": " + (block(v, depth + 1) if k in keys else json.dumps(v, sort_keys=True)) for k, v in sorted(d.items()))

    def block(v, depth):
        if isinstance(v, dict):
            return "{\n" + entries(v, depth) + "\n" + " " * (depth - 1) + "}"
        return "[\n" + ",\n".join(" " * depth + json.dumps(x) for x in v) + "\n" + " " * (depth - 1) + "]"
    f.write(block(doc, 1) + "\n")
