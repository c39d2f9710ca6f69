"""Fused finite-difference Greeks on Sobol paths (olmc_asian_qmc_greeks_fd / olmc_extrema_qmc_greeks_fd) without a device: the ABI
exports and binds them, every refusal comes before any device work, and ExoticAdapter picks the fused plan for a seeded method="qmc"
option only."""

import pytest

import optionslab_amd as ol
from optionslab_amd import _hip
from optionslab_amd.exceptions import GreeksError
from optionslab_amd.greeks import ExoticAdapter, compute_greeks_unified
from tests.abi_support import library, _out9, refused, sobol as _sobol

NAMES = ("olmc_asian_qmc_greeks_fd", "olmc_extrema_qmc_greeks_fd")
S, K, T, R, SIG = 100.0, 100.0, 1.0, 0.05, 0.2

_G = (S, K, T, R, SIG, 0.0, 1)                  # S K T r sigma q is_call
_GT0 = (S, K, 0.0, R, SIG, 0.0, 1)              # T = 0


def test_the_library_exports_and_binds_both_entry_points(library):
    for name in NAMES:
        assert hasattr(library, name)
        assert name in _hip.PROTOTYPES
    assert callable(_hip.asian_qmc_greeks_fd) and callable(_hip.extrema_qmc_greeks_fd)


_BRIDGE_CAP = "the Brownian-bridge construction takes at most OLMC_QMC_BRIDGE_MAX_STEPS (1024) dates"
_BITS = "only 30-bit Sobol tables (SciPy's default) are supported"
_REFUSALS = [
    # asian: ... avg_kind construction n_points n_steps sv shift bits antithetic second_order out9 evals
    ("olmc_asian_qmc_greeks_fd", lambda: (*_GT0, 0, 1, 64, 4, *_sobol(4), 30, 0, 0, _out9(), None), "T must be > 0"),
    ("olmc_asian_qmc_greeks_fd", lambda: (*_G, 2, 1, 64, 4, *_sobol(4), 30, 0, 0, _out9(), None),
     "bad avg_kind (arithmetic or geometric: the fp32-exponent form has no Sobol path)"),
    ("olmc_asian_qmc_greeks_fd", lambda: (*_G, 0, 2, 64, 4, *_sobol(4), 30, 0, 0, _out9(), None), "bad construction"),
    ("olmc_asian_qmc_greeks_fd", lambda: (*_G, 0, 1, 64, 1025, *_sobol(1025), 30, 0, 0, _out9(), None), _BRIDGE_CAP),
    ("olmc_asian_qmc_greeks_fd", lambda: (*_G, 1, 0, 64, 4, *_sobol(4), 29, 0, 0, _out9(), None), _BITS),
    ("olmc_asian_qmc_greeks_fd", lambda: (*_G, 0, 1, 0, 4, *_sobol(4), 30, 0, 0, _out9(), None), "n_paths must be >= 1"),
    ("olmc_asian_qmc_greeks_fd", lambda: (*_G, 0, 0, (1 << 30) + 1, 4, *_sobol(4), 30, 0, 0, _out9(), None), "at most 2**30 Sobol points"),
    ("olmc_asian_qmc_greeks_fd", lambda: (*_G, 0, 0, 64, 21202, *_sobol(4), 30, 0, 0, _out9(), None), "dims must be in [1, 21201]"),
    ("olmc_asian_qmc_greeks_fd", lambda: (*_G, 0, 1, 64, 4, *_sobol(4), 30, 0, 0, None, None), "null pointer"),
    ("olmc_asian_qmc_greeks_fd", lambda: (*_G, 0, 1, 64, 4, None, None, 30, 0, 0, _out9(), None), "null pointer"),
    # extrema: ... payoff barrier construction n_points n_steps sv shift bits antithetic second_order out9 evals
    ("olmc_extrema_qmc_greeks_fd", lambda: (*_GT0, 4, 0.0, 1, 64, 4, *_sobol(4), 30, 0, 0, _out9(), None), "T must be > 0"),
    ("olmc_extrema_qmc_greeks_fd", lambda: (*_G, 6, 120.0, 1, 64, 4, *_sobol(4), 30, 0, 0, _out9(), None), "bad payoff"),
    ("olmc_extrema_qmc_greeks_fd", lambda: (*_G, -1, 120.0, 1, 64, 4, *_sobol(4), 30, 0, 0, _out9(), None), "bad payoff"),
    ("olmc_extrema_qmc_greeks_fd", lambda: (*_G, 2, 0.0, 1, 64, 4, *_sobol(4), 30, 0, 0, _out9(), None), "Barrier must be positive"),
    ("olmc_extrema_qmc_greeks_fd", lambda: (*_G, 1, float("nan"), 1, 64, 4, *_sobol(4), 30, 0, 0, _out9(), None), "Barrier must be positive"),
    ("olmc_extrema_qmc_greeks_fd", lambda: (*_G, 5, 0.0, 7, 64, 4, *_sobol(4), 30, 0, 0, _out9(), None), "bad construction"),
    ("olmc_extrema_qmc_greeks_fd", lambda: (*_G, 4, 0.0, 1, 64, 2000, *_sobol(2000), 30, 1, 1, _out9(), None), _BRIDGE_CAP),
    ("olmc_extrema_qmc_greeks_fd", lambda: (*_G, 0, 120.0, 0, 64, 4, *_sobol(4), 31, 0, 0, _out9(), None), _BITS),
    ("olmc_extrema_qmc_greeks_fd", lambda: (*_G, 4, 0.0, 0, 0, 4, *_sobol(4), 30, 0, 0, _out9(), None), "n_paths must be >= 1"),
    ("olmc_extrema_qmc_greeks_fd", lambda: (*_G, 4, 0.0, 0, 1 << 31, 4, *_sobol(4), 30, 0, 0, _out9(), None), "at most 2**30 Sobol points"),
    ("olmc_extrema_qmc_greeks_fd", lambda: (*_G, 4, 0.0, 1, 64, 4, *_sobol(4), 30, 0, 0, None, None), "null pointer"),
]


@pytest.mark.parametrize("name,args,message", _REFUSALS, ids=[f"{n}-{i}" for i, (n, _a, _m) in enumerate(_REFUSALS)])
def test_refusals_answer_err_arg_before_any_device_work(library, name, args, message):
    refused(library, getattr(library, name)(*args()), message)


# ------------------------------------------------------------------------------------------------- the adapter's plan ----
class _Called(Exception):
    pass


@pytest.fixture
def stubbed(monkeypatch):
    """The device entry points record their call instead of running; the literal form's price() calls are refused loudly."""
    calls = []

    def fused(name):
        def f(*a, **k):
            calls.append(name)
            return [0.0] * 9, []
        return f

    def literal(*a, **k):
        raise _Called("a literal pricing call reached the device")

    for name in ("asian_qmc_greeks_fd", "extrema_qmc_greeks_fd", "asian_greeks_fd", "extrema_greeks_fd"):
        monkeypatch.setattr(_hip, name, fused(name))
    for name in ("lib", "asian_qmc", "extrema_qmc", "asian", "barrier", "lookback"):
        monkeypatch.setattr(_hip, name, literal)
    return calls


def _seeded(seed=5):
    return [
        (ol.AsianOption(S, K, T, R, SIG, seed=seed), {}, "asian_qmc_greeks_fd"),
        (ol.AsianOption(S, K, T, R, SIG, seed=seed), {"avg_type": "geometric", "path_construction": "sequential"}, "asian_qmc_greeks_fd"),
        (ol.BarrierOption(S, K, T, R, SIG, seed=seed, barrier=120.0), {"barrier_type": "up-and-in"}, "extrema_qmc_greeks_fd"),
        (ol.LookbackOption(S, K, T, R, SIG, seed=seed), {"lookback_type": "fixed", "antithetic": True}, "extrema_qmc_greeks_fd"),
    ]


@pytest.mark.parametrize("second_order", [False, True])
def test_a_seeded_qmc_option_takes_the_fused_plan(stubbed, second_order):
    for opt, kw, entry in _seeded():
        ad = ExoticAdapter(opt, n_paths=1000, n_steps=16, method="qmc", **kw)
        plan = ad._fused_plan()
        assert plan is not None and plan[-1] is True
        stubbed.clear()
        out = compute_greeks_unified(ad, S, K, T, R, SIG, "call", 0.0, include_second_order=second_order)
        assert stubbed == [entry]
        assert len(out) == (9 if second_order else 6)


def test_an_unseeded_qmc_option_takes_the_literal_form(stubbed):
    for opt, kw, _entry in _seeded(seed=None):
        ad = ExoticAdapter(opt, n_paths=1000, n_steps=16, method="qmc", **kw)
        assert ad._fused_plan() is None
        with pytest.raises(GreeksError, match="literal pricing call"):
            compute_greeks_unified(ad, S, K, T, R, SIG, "call", 0.0)
        assert stubbed == []


def test_fused_false_keeps_the_literal_form(stubbed):
    opt, kw, _entry = _seeded()[0]
    with pytest.raises(GreeksError, match="literal pricing call"):
        compute_greeks_unified(ExoticAdapter(opt, n_paths=1000, n_steps=16, method="qmc", **kw), S, K, T, R, SIG, fused=False)
    assert stubbed == []


@pytest.mark.parametrize("fused", [True, None, False])
def test_qmc_with_fp32_precision_is_refused_as_the_literal_form_refuses_it(stubbed, fused):
    ad = ExoticAdapter(ol.AsianOption(S, K, T, R, SIG, seed=5), n_paths=1000, n_steps=16, method="qmc", precision="fp32")
    with pytest.raises(GreeksError, match="fp64 only") as e:
        compute_greeks_unified(ad, S, K, T, R, SIG, "call", fused=fused)
    assert isinstance(e.value.__cause__, ValueError)
    assert stubbed == []


def test_the_literal_forms_table_refusals_hold_on_the_fused_path(stubbed):
    ad = ExoticAdapter(ol.LookbackOption(S, K, T, R, SIG, seed=5), n_paths=1000, n_steps=2000, method="qmc")
    assert ad._fused_plan() is not None
    with pytest.raises(GreeksError, match="1024") as e:
        compute_greeks_unified(ad, S, K, T, R, SIG, "call", fused=True)
    assert isinstance(e.value.__cause__, ValueError)
    assert stubbed == []


def test_a_pseudo_random_option_keeps_its_fused_plan(stubbed):
    ad = ExoticAdapter(ol.BarrierOption(S, K, T, R, SIG, seed=5, barrier=120.0), n_paths=1000, n_steps=16)
    assert ad._fused_plan()[-1] is False
    compute_greeks_unified(ad, S, K, T, R, SIG, "call")
    assert stubbed == ["extrema_greeks_fd"]
