"""What tests/test_heston_american_cpu.py and tests/test_gpu_heston_american.py share: the refusal rows of include/olha.h.  A helper, not a
test module.  The rows are the assertions; tests.abi_support.refused is their runner.  Every row is refused before any device work, so
the CPU file runs them without a device and the GPU file on an initialised one.
"""
import ctypes as C

from tests.abi_support import _ST, sobol

CONTRACT = (100.0, 100.0, 1.0, 0.05, 0.0, 0)                      # S K T r q is_call
USUAL = (2.0, 0.04, 0.3, -0.7, 0.04)                               # kappa theta sigma_v rho v0
EULER, QE = 0, 1
SPOT_VARIANCE, SPOT = 0, 1
SEQUENTIAL, BRIDGE = 0, 1
TOO_BIG = "path matrices would exceed 64 GB: lower n_paths or n_steps"
DEGREE_SV = "poly_degree must be in [1, 3] for OLHA_BASIS_SPOT_VARIANCE"
DEGREE_S = "poly_degree must be in [1, 4] for OLHA_BASIS_SPOT"
QE_BRIDGE = "the QE scheme takes OLMC_QMC_SEQUENTIAL only: its variance draw is a uniform, not a Brownian increment"
TWO_DIMS = "n_steps must be in [1, 10600]: a step takes two of the 21201 Sobol dimensions"
BITS = "only 30-bit Sobol tables (SciPy's default) are supported"


def _model(**changed):
    m = dict(zip(("kappa", "theta", "sigma_v", "rho", "v0"), USUAL))
    m.update(changed)
    return tuple(m.values())


def _philox(model=USUAL, scheme=EULER, basis=SPOT_VARIANCE, degree=2, n_paths=100, n_steps=4, out=True):
    return lambda: (*CONTRACT, *model, scheme, basis, degree, n_paths, n_steps, 1, _ST() if out else None)


def _sobol(model=USUAL, scheme=EULER, basis=SPOT_VARIANCE, degree=2, construction=SEQUENTIAL, n_points=64, dims=8, bits=30, sv=True, shift=True, out=True):
    def args():
        tables = sobol(dims)
        return (*CONTRACT, *model, scheme, basis, degree, construction, n_points, tables[0] if sv else None, tables[1] if shift else None, dims, bits,
                _ST() if out else None)
    return args


def _scales(n_steps=4, last=True):
    def args():
        a = [(C.c_double * (max(n_steps, 1) + 1))() for _ in range(4)]
        return (*CONTRACT, *USUAL[:3], USUAL[4], n_steps, a[0], a[1], a[2], a[3] if last else None)
    return args


REFUSALS = [
    ("olha_american_lsm", _philox(out=False), "null pointer"),
    ("olha_american_lsm", _philox(scheme=2), "bad scheme (OLHA_EULER or OLHA_QE)"),
    ("olha_american_lsm", _philox(basis=2), "bad basis (OLHA_BASIS_SPOT_VARIANCE or OLHA_BASIS_SPOT)"),
    ("olha_american_lsm", _philox(degree=0), DEGREE_SV),
    ("olha_american_lsm", _philox(degree=4), DEGREE_SV),
    ("olha_american_lsm", _philox(basis=SPOT, degree=0), DEGREE_S),
    ("olha_american_lsm", _philox(basis=SPOT, degree=5), DEGREE_S),
    ("olha_american_lsm", _philox(_model(rho=1.5)), "rho must be in [-1, 1]"),
    ("olha_american_lsm", _philox(_model(rho=float("nan"))), "rho must be in [-1, 1]"),
    ("olha_american_lsm", _philox(_model(kappa=0.0), scheme=QE), "kappa must be positive for the QE scheme"),
    ("olha_american_lsm", _philox(_model(theta=0.0), scheme=QE), "theta must be positive for the QE scheme"),
    ("olha_american_lsm", _philox(_model(sigma_v=0.0), scheme=QE), "sigma_v must be positive for the QE scheme"),
    ("olha_american_lsm", _philox(_model(v0=-0.01), scheme=QE), "v0 must be non-negative for the QE scheme"),
    ("olha_american_lsm", _philox(n_paths=0), "n_paths must be >= 1"),
    ("olha_american_lsm", _philox(n_steps=0), "n_steps must be >= 1"),
    ("olha_american_lsm", _philox(n_paths=5 * 10 ** 8, n_steps=10), TOO_BIG),
    ("olha_american_lsm", _philox(basis=SPOT, degree=3, n_paths=5 * 10 ** 8, n_steps=10), TOO_BIG),
    # two faults at once: the refusal is the one of the check that comes first
    ("olha_american_lsm", _philox(scheme=2, degree=9, out=False), "null pointer"),
    ("olha_american_lsm", _philox(scheme=2, basis=2, degree=9), "bad scheme (OLHA_EULER or OLHA_QE)"),
    ("olha_american_lsm", _philox(_model(rho=2.0), degree=9, n_paths=0), DEGREE_SV),
    ("olha_american_lsm", _philox(_model(rho=2.0), n_paths=0), "rho must be in [-1, 1]"),
    ("olha_american_lsm_qmc", _sobol(out=False), "null pointer"),
    ("olha_american_lsm_qmc", _sobol(sv=False), "null pointer"),
    ("olha_american_lsm_qmc", _sobol(shift=False), "null pointer"),
    ("olha_american_lsm_qmc", _sobol(scheme=-1), "bad scheme (OLHA_EULER or OLHA_QE)"),
    ("olha_american_lsm_qmc", _sobol(basis=-1), "bad basis (OLHA_BASIS_SPOT_VARIANCE or OLHA_BASIS_SPOT)"),
    ("olha_american_lsm_qmc", _sobol(degree=4), DEGREE_SV),
    ("olha_american_lsm_qmc", _sobol(basis=SPOT, degree=5), DEGREE_S),
    ("olha_american_lsm_qmc", _sobol(dims=7), "dims must be even: a step takes two Sobol dimensions"),
    ("olha_american_lsm_qmc", _sobol(_model(rho=-1.5)), "rho must be in [-1, 1]"),
    ("olha_american_lsm_qmc", _sobol(_model(sigma_v=0.0), scheme=QE), "sigma_v must be positive for the QE scheme"),
    ("olha_american_lsm_qmc", _sobol(scheme=QE, construction=BRIDGE), QE_BRIDGE),
    ("olha_american_lsm_qmc", _sobol(construction=2), "bad construction"),
    ("olha_american_lsm_qmc", _sobol(construction=BRIDGE, dims=2050), "the Brownian-bridge construction takes at most OLMC_QMC_BRIDGE_MAX_STEPS (1024) dates"),
    ("olha_american_lsm_qmc", _sobol(dims=0), TWO_DIMS),
    ("olha_american_lsm_qmc", _sobol(bits=31), BITS),
    ("olha_american_lsm_qmc", _sobol(n_points=0), "n_paths must be >= 1"),
    ("olha_american_lsm_qmc", _sobol(n_points=(1 << 30) + 1), "at most 2**30 Sobol points"),
    ("olha_american_lsm_qmc", _sobol(n_points=1 << 29, dims=20), TOO_BIG),
    ("olha_american_lsm_qmc", _sobol(scheme=QE, construction=BRIDGE, bits=31, n_points=0), QE_BRIDGE),
    ("olha_regressor_scales", _scales(last=False), "null pointer"),
    ("olha_regressor_scales", _scales(n_steps=0), "n_steps must be >= 1"),
]
REFUSAL_IDS = [f"{name}-{i}" for i, (name, _args, _message) in enumerate(REFUSALS)]
