"""The run plumbing the GPU tests share: a problem's arrays, an environment variable held for one call, the handle's options as
vectors and keywords, the solve and option builders, and the in-process loopback communicator with its ranks.  (The numpy
reference of the LM terms is tests/_lm_ref.py.)"""
import contextlib
import ctypes as C
import os
import threading

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOOPBACK = os.path.join(ROOT, "tests", "helpers", "libba_loopback.so")


def arrays(p):
    return (p["cam_idx1"], p["pnt_idx1"], p["pt2d"], p["x0"], p["ncams"], p["npnts"], p["nobs"])


def env(name, value, fn):
    """fn() with the environment variable set to value (None: unset), the variable restored afterwards"""
    old = os.environ.get(name)
    if value is None:
        os.environ.pop(name, None)
    else:
        os.environ[name] = value
    try:
        return fn()
    finally:
        if old is None:
            os.environ.pop(name, None)
        else:
            os.environ[name] = old


# ---- the handle's options as vectors and keywords -------------------------------------------------------------------------
def fixed_vector(ba, p, kw):
    """boolean over x = [points; cameras]: True where the options of kw fix the entry"""
    cam, pnt = ba._lib.fixed_masks(p["ncams"], p["npnts"], kw.get("fixed_cameras"), kw.get("fixed_points"),
                                   kw.get("fixed_camera_params"))
    fixed_p = np.repeat(pnt.astype(bool), 3)
    fixed_c = ((cam[:, None] >> np.arange(9)) & 1).astype(bool).ravel()
    return np.concatenate([fixed_p, fixed_c])


def gauge_kw(p):
    """camera 1's pose (r, t) and the first translation component of camera 2: the 7 DoF of a similarity transform"""
    comp = np.zeros((p["ncams"], 9), dtype=bool)
    comp[0, :6] = True
    comp[1, 3] = True
    return dict(fixed_camera_params=comp)


def solve(ba, m, variant=1, facto="LDL", normalize="None", **kw):
    args = (facto, "AMD", normalize) + ((False,) if variant == 1 else ())
    return ba.Levenberg_Marquardt(ba.FeasibilityResidual(m), *args, **kw)


def lm_opts(ba, **kw):
    """ba_lm_opts with every field at its default (lm.jl's variant, :LDL, :AMD), then the fields of kw"""
    o = ba._lib.LMOpts(variant=1, facto=0, normalize=0, linesearch=0, facto_type=0, ite_max=-1, verbose=0, x_f32=0, restol=-1,
                       satol=-1, srtol=-1, oatol=-1, ortol=-1, atol=-1, rtol=-1, nu_d=-1, nu_m=-1, lam=-1, delta_d=-1, max_time=-1,
                       pcg_tol=-1, pcg_max_iter=-1, perm=0)
    for k, v in kw.items():
        setattr(o, k, v)
    return o


# ---- several ranks in one process over the stream-ordered loopback transport (tests/helpers/ba_loopback.hip) -----------------
_loopback_lib = None


def loopback_lib():
    """the loopback transport's library, its ctypes signatures declared"""
    global _loopback_lib
    if _loopback_lib is None:
        assert os.path.exists(LOOPBACK), f"{LOOPBACK} is missing: __graft_entry__.build() compiles it"
        L = C.CDLL(LOOPBACK)
        L.ba_loopback_create.restype = C.c_void_p
        L.ba_loopback_create.argtypes = [C.c_int, C.c_size_t]
        L.ba_loopback_destroy.argtypes = [C.c_void_p]
        L.ba_loopback_rank.restype = C.c_void_p
        L.ba_loopback_rank.argtypes = [C.c_void_p, C.c_int]
        L.ba_loopback_ops.restype = C.c_long
        L.ba_loopback_ops.argtypes = [C.c_void_p]
        _loopback_lib = L
    return _loopback_lib


@contextlib.contextmanager
def loopback_world(world, stage_bytes):
    """(library, communicator) of `world` ranks with stage_bytes of staging each; destroyed on exit"""
    L = loopback_lib()
    loop = L.ba_loopback_create(world, stage_bytes)
    assert loop, "loopback communicator could not be created"
    try:
        yield L, loop
    finally:
        L.ba_loopback_destroy(loop)


def attach_loopback(ba, m, L, loop, rank, world):
    """rank `rank` of the communicator as the handle's transport (before the handle's first solve)"""
    hook = C.cast(L.ba_loopback_hook, ba._lib.COMM_CB)
    ba._lib.check(ba._lib.lib().ba_lm_set_comm_hook(m.handle, rank, world, hook, L.ba_loopback_rank(loop, rank)))


@pytest.fixture(scope="module")
def loopback(gpu_ok):
    return loopback_lib()


class Ranks:
    """`world` shards of one problem as handles in this process, attached to one loopback communicator."""

    def __init__(self, ba, L, prob, world, stage_mb=64):
        self.ba, self.L, self.world, self.prob = ba, L, world, prob
        whole = ba.synthetic.as_arrays(prob)
        self.loop = L.ba_loopback_create(world, stage_mb << 20)
        assert self.loop, "loopback communicator could not be created"
        self.shards, self.models = [], []
        for r in range(world):
            local, info = ba.parallel.shard_problem(whole, r, world)
            m = ba.BALNLPModel(arrays=local, device=0)
            attach_loopback(ba, m, L, self.loop, r, world)
            self.shards.append((local, info))
            self.models.append(m)

    def step(self, lam, **kw):
        """one sharded LM step, every rank on its own host thread -> (global delta from rank 0's cameras, per-rank camera
        parts, model value)"""
        out, err = [None] * self.world, [None] * self.world

        def run(r):
            try:
                out[r] = self.ba.lm_step(self.models[r], self.shards[r][0][3], lam, **kw)
            except Exception as e:  # noqa: BLE001 -- reported below with the rank
                err[r] = e

        ts = [threading.Thread(target=run, args=(r,)) for r in range(self.world)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        bad = [(r, e) for r, e in enumerate(err) if e is not None]
        assert not bad, f"rank(s) failed: {bad}"
        ncams, npnts = self.prob["ncams"], self.prob["npnts"]
        delta = np.zeros(3 * npnts + 9 * ncams)
        cams = []
        for r in range(self.world):
            pb, pe = self.shards[r][1]["point_range"]
            d = out[r][0]
            delta[3 * pb:3 * pe] = d[:3 * (pe - pb)]
            cams.append(d[3 * (pe - pb):].copy())
        delta[3 * npnts:] = cams[0]
        return delta, cams, out[0][1]

    def close(self):
        for m in self.models:
            m.close()
        self.L.ba_loopback_destroy(self.loop)
