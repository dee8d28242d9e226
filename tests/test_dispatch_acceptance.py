"""Which descriptors the library accepts, pinned against a recording (tests/golden/dispatch_acceptance.json): for every descriptor of a
fixed enumeration, whether corbo_hip_get_dims accepts it (host-only: build_structure) and whether corbo_hip_create refuses it with
CORBO_HIP_ERR_UNSUPPORTED -- the device-kernel gate, which runs before any HIP call.  The device index passed is out of range, so nothing
is allocated on a machine with or without a GPU.

The enumeration covers every public dynamics id, every registered user slot and one empty one, every shape of the model table
(csrc/model_table.inc) and its neighbours in nx +- 1 and nu +- 1, every valid (grid, defect) pair -- fixed dt on the FiniteDifferencesGrid /
MultipleShootingGrid, free dt on their variable twins -- and horizons on both sides of 256 and of 1024.

`python tests/test_dispatch_acceptance.py` rewrites the fixture from the library capi.load() finds (CORBO_HIP_LIB selects another build;
the fixture names the commit checked out, which should be the one that library was built from)."""
import ctypes as C
import json
import os
import subprocess

from control_box_rst_amd import capi, problems

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "dispatch_acceptance.json")

TABLE_SHAPES = [(2, 1), (2, 2), (3, 1), (3, 2), (3, 3), (4, 1), (12, 4), (6, 2)]   # model_table.inc and the registered user models
DYNAMICS = list(range(capi.DYN_LINEAR_STATE_SPACE + 1)) + [capi.DYN_USER + 0, capi.DYN_USER + 1, capi.DYN_USER + 2]
GRID_DEFECT = [(g, dfx) for g in (capi.GRID_FD, capi.GRID_FD_VARIABLE)
               for dfx in (capi.DEFECT_FORWARD, capi.DEFECT_BACKWARD, capi.DEFECT_MIDPOINT, capi.DEFECT_CRANK_NICOLSON)] + \
              [(capi.GRID_MS, capi.DEFECT_RK4_SHOOTING), (capi.GRID_MS_VARIABLE, capi.DEFECT_RK4_SHOOTING)]
HORIZONS = [12, 256, 257, 1024, 1025]
DEVICE_OUT_OF_RANGE = 1 << 20
ERR_UNSUPPORTED = -3   # CORBO_HIP_ERR_UNSUPPORTED (include/corbo_hip.h)


def shapes():
    out = set()
    for nx, nu in TABLE_SHAPES:
        out |= {(nx, nu), (nx - 1, nu), (nx + 1, nu), (nx, nu - 1), (nx, nu + 1)}
    return sorted((nx, nu) for nx, nu in out if nx >= 1 and nu >= 1)


def descriptor(dyn, nx, nu, grid, defect, N):
    free_dt = grid in (capi.GRID_FD_VARIABLE, capi.GRID_MS_VARIABLE)
    d = problems.make_desc(grid=grid, defect=defect, dynamics=dyn, nx=nx, nu=nu, N=N, dt=0.1, q=(1.0,) * nx, r=(0.1,) * nu, qf=(10.0,) * nx,
                           u_lb=(-1.0,) * nu, u_ub=(1.0,) * nu, dyn_params=(1.0,), **(dict(dt_lb=0.01, dt_ub=10.0) if free_dt else {}))
    if nx * nx <= len(d.lin_a) and nx * nu <= len(d.lin_b):   # (LinearStateSpaceModel: A = -I, B = [I 0])
        for i in range(nx):
            d.lin_a[i * nx + i] = -1.0
        for i in range(min(nx, nu)):
            d.lin_b[i * nu + i] = 1.0
    return d


LEGEND = ('"dyn nx nu": one character per (grid, defect) pair and horizon, grid_defect-major; "-" get_dims refuses, "U" get_dims accepts and '
          'create refuses with CORBO_HIP_ERR_UNSUPPORTED, "+" get_dims accepts and create gets past the gate')


def acceptance(lib):
    """{"dyn nx nu": codes} as LEGEND describes."""
    out = {}
    dims = capi.Dims()
    for dyn in DYNAMICS:
        for nx, nu in shapes():
            codes = []
            for grid, defect in GRID_DEFECT:
                for N in HORIZONS:
                    d = descriptor(dyn, nx, nu, grid, defect, N)
                    if lib.corbo_hip_get_dims(C.byref(d), C.byref(dims)) != 0:
                        codes.append("-")
                        continue
                    h = C.c_void_p()
                    rc = lib.corbo_hip_create(C.byref(d), 1, DEVICE_OUT_OF_RANGE, C.byref(h))
                    assert rc != 0 and not h.value, (dyn, nx, nu, grid, defect, N, rc)
                    codes.append("U" if rc == ERR_UNSUPPORTED else "+")
            out[f"{dyn} {nx} {nu}"] = "".join(codes)
    return out


def test_dispatch_acceptance_matches_recording():
    """The device-kernel gate (kernels.hip device_kernels_exist and the factor sizes corbo_hip_create checks) and the structure validation
    accept exactly the descriptors they accepted when the fixture was recorded."""
    g = json.load(open(FIXTURE))
    assert (g["dynamics"], [list(s) for s in g["shapes"]], [list(p) for p in g["grid_defect"]], g["horizons"]) == \
           (DYNAMICS, [list(s) for s in shapes()], [list(p) for p in GRID_DEFECT], HORIZONS)
    got = acceptance(capi.load())
    assert sum(c == "+" for v in got.values() for c in v) > 0 and sum(c == "U" for v in got.values() for c in v) > 0
    diff = {k: (g["acceptance"][k], v) for k, v in got.items() if g["acceptance"].get(k) != v}
    assert not diff, diff


if __name__ == "__main__":
    rev = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip()
    rec = {"recorded_with": f"the library built from commit {rev}", "legend": LEGEND, "dynamics": DYNAMICS, "shapes": shapes(),
           "grid_defect": GRID_DEFECT, "horizons": HORIZONS}
    acc = acceptance(capi.load())
    with open(FIXTURE, "w") as f:
        f.write("{\n" + "".join(f"{json.dumps(k)}: {json.dumps(v)},\n" for k, v in rec.items()) + '"acceptance": {\n' +
                ",\n".join(f"  {json.dumps(k)}: {json.dumps(v)}" for k, v in acc.items()) + "\n}\n}\n")
