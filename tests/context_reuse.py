"""What tests/test_gpu_context_reuse.py drives a long-lived context with: the raw C ABI of include/rtgpu.h behind a thin wrapper (Context), a State -- everything
that decides what rtgpu_render_pass renders: scene, camera, frame size, integrator, shard, the viewport's pass settings -- the oracle's buffers for a state,
computed once per state name and left unchanged, and the probe: three passes on the context as it stands, compared with them word for word.

The oracle side needs no device: oracle_of() and check_oracle() run on a CPU-only machine, which is where the "not empty" and "differs from the state before"
conditions of every state list of the test file are asserted first (check_all_state_lists)."""
import ctypes as C

import numpy as np

import oracle_lib
import raytracer_amd as ra

OK, INVALID_ARGUMENT, NOT_READY, UNSUPPORTED = 0, -1, -5, -6
MIS, VCM, PATH_TRACER, DEBUG, LIGHT_TRACER = 0, 1, 2, 3, 4   # RtIntegrator
PASSES = 3
COMPARED = ("numRays", "numShadowRays", "numShadowRaysHit", "numPrimaryRays", "numRayBoxTests", "numPassedRayBoxTests", "numRayTriangleTests",
            "numPassedRayTriangleTests", "numMeshHits", "numAnalyticHits", "numShadowRayBoxTests", "numShadowRayTriangleTests")
NOT_INTERSECTION = ("numRays", "numShadowRays", "numShadowRaysHit", "numPrimaryRays", "numMeshHits", "numAnalyticHits")


class WalkInfo(C.Structure):
    _fields_ = [("kernel", C.c_uint32), ("reserved", C.c_uint32), ("nodeBytes", C.c_uint64), ("leafBoxBytes", C.c_uint64), ("triangleBytes", C.c_uint64)]


class Shard(C.Structure):   # RtgpuShard, passed by value
    _fields_ = [("rank", C.c_uint32), ("worldSize", C.c_uint32)]


def words(a):
    return np.ascontiguousarray(a).view(np.uint32)


_blue_noise = None


def with_blue_noise(scene):
    """the scene's descriptor with the blue-noise table in it, as run_both of the parity tests sets it"""
    global _blue_noise
    if _blue_noise is None:
        _blue_noise = ra.load_blue_noise()
    scene.desc.contents.blueNoise = _blue_noise.ctypes.data
    return scene.desc


class State:
    """`name` keys the oracle's buffers: one name, one state.  vp_args are ra.Viewport's (seed, max_ray_depth, min_russian_roulette_depth, light_sampling_all,
    dimensions ...); vcm: the keyword settings of oracle_lib.Vcm; debug_mode: a DebugRenderingMode"""

    def __init__(self, name, scene, camera, w, h, integrator=MIS, shard=(0, 1), vcm=None, debug_mode=None, **vp_args):
        self.name, self.scene, self.camera, self.w, self.h = name, scene, camera, w, h
        self.integrator, self.shard, self.vcm, self.debug_mode = integrator, shard, vcm, debug_mode
        self.vp_args = dict(seed=99, **vp_args) if "seed" not in vp_args else dict(vp_args)
        self._params = None

    def params(self, n=PASSES):
        """the constants of passes 0 .. n - 1, from a viewport without a renderer: the sample sequence depends on the seed and the settings alone.  Each pass is
        finished as Viewport::Render finishes it (rth_viewport_finish_pass), so that the next one gets its own passIndex -- the secondary buffer takes the even
        passes, the bidirectional integrator restarts at 0 -- and its own per-pixel generator key"""
        if self._params is None or len(self._params) < n:
            vp = ra.Viewport(self.w, self.h, **self.vp_args)
            self._params = []
            for _ in range(max(n, PASSES + 2)):
                self._params.append(vp.next_pass_params(self.camera))
                ra.host_lib().rth_viewport_finish_pass(vp._h)
            assert [p.passIndex for p in self._params] == list(range(len(self._params)))
        return self._params[:n]

    def vcm_words(self):
        return oracle_lib.Vcm(**self.vcm).settings   # the 28 words of RtVcmParams


_oracle = {}


def oracle_of(state, n=PASSES):
    """dict(sum, secondary, counters: name -> int, photons: the VCM photon count after every pass) of `n` passes of the state on a fresh film"""
    key = (state.name, n)
    if key in _oracle:
        assert _oracle[key]["state"] is state, "two states share the name %r" % (state.name,)
        return _oracle[key]
    desc, w, h = with_blue_noise(state.scene), state.w, state.h
    ref, ref2 = np.zeros((h, w, 3), dtype=np.float32), np.zeros((h, w, 3), dtype=np.float32)
    cnt, photons = np.zeros(16, dtype=np.uint64), []
    vcm = oracle_lib.Vcm(**state.vcm) if state.integrator == VCM else None
    light = np.zeros((h, w, 3), dtype=np.float32)
    for i, p in enumerate(state.params(n)):
        if state.integrator in (MIS, PATH_TRACER):
            oracle_lib.render_pass(desc, p, w, h, ref, ref2, cnt, shard=state.shard, threads=8, plain=state.integrator == PATH_TRACER)
        elif state.integrator == DEBUG:
            oracle_lib.render_pass_debug(desc, p, w, h, state.debug_mode, ref, ref2, cnt, threads=8)
        elif state.integrator == LIGHT_TRACER:
            oracle_lib.light_tracer_pass(desc, p, w, h, ref, ref2 if i % 2 == 0 else None, cnt)
        else:
            vcm.render_pass(desc, p, w, h, ref, ref2 if i % 2 == 0 else None, light, cnt)
            photons.append(vcm.num_photons())
    for a in (ref, ref2):
        a.setflags(write=False)
    assert not light.any() or state.vcm.get("camera_connecting_weight", 1.0) != 0.0
    _oracle[key] = dict(state=state, sum=ref, secondary=ref2, counters={name: int(cnt[i]) for i, name in enumerate(ra.COUNTER_NAMES)}, photons=photons)
    return _oracle[key]


def check_oracle(state, previous=None, n=PASSES):
    """What keeps a probe from passing vacuously, on the oracle's images alone: the frame has lit pixels, and it is not the frame of the state before"""
    want = oracle_of(state, n)
    assert np.isfinite(want["sum"]).all() and want["sum"].any() and want["secondary"].any(), "%s: the oracle's frame is empty" % state.name
    assert n < 2 or state.w * state.h == 1 or not np.array_equal(words(want["sum"]), words(want["secondary"])), "%s: the secondary buffer holds every pass" % state.name
    if previous is not None:
        before = oracle_of(previous, n)["sum"]
        assert before.shape != want["sum"].shape or not np.array_equal(words(before), words(want["sum"])), \
            "%s: the oracle's frame is the frame of %s" % (state.name, previous.name)
    return want


def check_state_list(states):
    """states: [(State, differs from the one before)] in the order a test visits them"""
    previous = None
    for state, differs in states:
        check_oracle(state, previous if differs else None)
        previous = state


class Context:
    """An RtgpuContext through the raw C ABI; every call asserts its status unless the test asks for it"""

    def __init__(self, walk="default"):
        self.lib = ra.rtgpu_lib()
        self.ctx = C.c_void_p()
        self.walk = walk
        assert self.lib.rtgpu_create(0, C.byref(self.ctx)) == OK, self.error()
        assert self.lib.rtgpu_set_intersection_counters(self.ctx, 1 if walk == "counting" else 0) == OK, self.error()

    def error(self):
        return (self.lib.rtgpu_last_error() or b"").decode()

    def close(self):
        if self.ctx:
            self.lib.rtgpu_destroy(self.ctx)
            self.ctx = None

    def upload(self, scene):
        assert self.lib.rtgpu_upload_scene(self.ctx, with_blue_noise(scene)) == OK, self.error()

    def resize(self, w, h):
        assert self.lib.rtgpu_resize(self.ctx, C.c_uint32(w), C.c_uint32(h)) == OK, self.error()

    def reset(self):
        assert self.lib.rtgpu_reset(self.ctx) == OK, self.error()

    def set_shard(self, rank, world):
        assert self.lib.rtgpu_set_shard(self.ctx, Shard(rank, world)) == OK, self.error()

    def set_integrator(self, state):
        vcm = state.vcm_words() if state.integrator == VCM else None
        assert self.lib.rtgpu_set_integrator(self.ctx, C.c_uint32(state.integrator), vcm.ctypes.data_as(C.c_void_p) if vcm is not None else None) == OK, self.error()
        if state.integrator == DEBUG:
            assert self.lib.rtgpu_set_debug_rendering_mode(self.ctx, C.c_uint32(state.debug_mode)) == OK, self.error()

    def render(self, p):
        assert self.lib.rtgpu_render_pass(self.ctx, C.byref(p)) == OK, self.error()

    def read(self, w, h):
        s, s2 = np.full((h, w, 3), np.nan, dtype=np.float32), np.full((h, w, 3), np.nan, dtype=np.float32)
        fp = C.POINTER(C.c_float)
        assert self.lib.rtgpu_read_sum(self.ctx, s.ctypes.data_as(fp), s2.ctypes.data_as(fp)) == OK, self.error()
        return s, s2

    def counters(self):
        raw = ra.RtCounters()
        assert self.lib.rtgpu_get_counters(self.ctx, C.byref(raw)) == OK, self.error()
        return {name: int(getattr(raw, name)) for name in ra.COUNTER_NAMES}

    def photons(self):
        n = C.c_uint32(0xFFFFFFFF)
        assert self.lib.rtgpu_vcm_num_photons(self.ctx, C.byref(n)) == OK, self.error()
        return int(n.value)

    def walk_info(self):
        wi = WalkInfo()
        assert self.lib.rtgpu_get_walk_info(self.ctx, C.byref(wi)) == OK, self.error()
        return (wi.kernel, wi.nodeBytes, wi.leafBoxBytes, wi.triangleBytes)


def assert_film(got, got2, want, what):
    for name, a, b in (("sum", got, want["sum"]), ("secondary", got2, want["secondary"])):
        assert a.shape == b.shape, (what, name, a.shape, b.shape)
        bad = np.argwhere(words(a) != words(b))
        assert len(bad) == 0, "%s, %s: %d of %d words differ from the oracle's, first at %r: %r, the oracle has %r" % (
            what, name, len(bad), b.size, tuple(bad[0]), a[tuple(bad[0])], b[tuple(bad[0])])


def assert_counters(before, after, want, walk, what):
    for name in (COMPARED if walk == "counting" else NOT_INTERSECTION):
        assert after[name] - before[name] == want["counters"][name], (what, name, after[name] - before[name], want["counters"][name])
    if walk != "counting":   # the reference's intersection counters belong to its own walk: off means untouched
        assert after["numRayBoxTests"] == before["numRayBoxTests"] and after["numRayTriangleTests"] == before["numRayTriangleTests"], what


def probe(ctx, state, previous=None, reset=True, n=PASSES):
    """`n` passes of `state` on the context as it stands -- no read-back in between -- against the oracle: both sum buffers word for word, the counters as the
    difference of two reads.  reset=False where the film is fresh (behind rtgpu_resize, rtgpu_set_shard)"""
    want = check_oracle(state, previous, n)
    if reset:
        ctx.reset()
    before = ctx.counters()
    for p in state.params(n):
        ctx.render(p)
    got, got2 = ctx.read(state.w, state.h)
    after = ctx.counters()
    assert_film(got, got2, want, state.name)
    assert_counters(before, after, want, ctx.walk, state.name)
    return got, got2
