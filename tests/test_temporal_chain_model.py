"""Properties of the model of temporal accumulation over chain guides (tests/temporal_chain_ref.py; include/rtgpu.h, "Temporal accumulation over chain guides")
that need no GPU: its identity with the existing models under k = 0, the geometry of the virtual position worked out analytically, each of the three rules on a
frame built for it, and the share of reflection pixels that find their history between two oracle recordings of the hall scene."""
import numpy as np
import pytest

import temporal_chain_ref as chain_ref
import temporal_clip_ref
import temporal_moving_ref
import temporal_ref
from temporal_ref import F

CLIP = dict(radius=2, gamma=1.0, min_count=4)


def words(a):
    return np.ascontiguousarray(a).view(np.uint32)


def assert_same_result(got, want, what):
    for have, expect, name in zip(got[:4], want[:4], ("history", "motion", "taken", "reason")):
        if name == "history":
            for key in ("a", "b", "length"):
                assert np.array_equal(words(have[key]), words(expect[key])), "%s: %s" % (what, key)
        else:
            assert np.array_equal(have, expect, equal_nan=True), "%s: %s" % (what, name)


def as_first_hit(cur):
    """the chain planes under which the chain call is the call without: k = 0, V = P, D = depth"""
    h, w = cur["depth"].shape
    return dict(virtual_position=cur["position"], chain_length=np.zeros((h, w), dtype=np.uint32), chain_distance=cur["depth"])


# ---- 1. identity ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clip", [None, CLIP], ids=["no_clip", "clip"])
def test_with_k_zero_the_model_is_the_models_without(clip):
    t = temporal_ref.random_temporal_frame(45, 23, seed=3)
    cur, history = t["current"], dict(t["history"], chain_length=np.zeros((23, 45), dtype=np.uint32))
    common = dict(prev_world_to_screen=t["prev_world_to_screen"], prev_sample_offset=t["prev_sample_offset"], color_scale=0.5)
    got = chain_ref.accumulate_chain(history=history, clip=clip, **cur, **as_first_hit(cur), **common)
    want = temporal_clip_ref.accumulate_clip(history=t["history"], clip=clip, **cur, **common)
    assert_same_result(got, want, "static")
    assert np.array_equal(words(got[4]["f"]), words(want[4]["f"])) and np.array_equal(got[4]["cnt"], want[4]["cnt"])
    if clip is None:
        assert_same_result(got, temporal_ref.accumulate(history=t["history"], **cur, **common), "temporal_ref")
    assert (got[3] == temporal_ref.BLENDED).sum() > 400 and not got[0]["chain_length"].any()
    # no history: every pixel starts, as ever
    assert_same_result(chain_ref.accumulate_chain(clip=clip, **cur, **as_first_hit(cur), color_scale=0.5), temporal_clip_ref.accumulate_clip(clip=clip, **cur, color_scale=0.5), "start")
    # objects given
    m = temporal_moving_ref.random_moving_frame(45, 23, seed=4)
    cur, history = m["current"], dict(m["history"], chain_length=np.zeros((23, 45), dtype=np.uint32))
    common = dict(prev_world_to_screen=m["prev_world_to_screen"], prev_sample_offset=m["prev_sample_offset"], object_motion=m["object_motion"])
    got = chain_ref.accumulate_chain(history=history, clip=clip, **cur, **as_first_hit(cur), **common)
    assert_same_result(got, temporal_clip_ref.accumulate_clip(history=m["history"], clip=clip, **cur, **common), "moving")
    assert (got[3] == temporal_ref.BLENDED).sum() > 300


# ---- 2. the geometry, analytically ---------------------------------------------------------------------------------------------------------------
W, H = 320, 180
OFFSET = (0.5, 0.5)


def pinhole(eye, yaw_deg, fov_deg=60.0):
    """(worldToScreen 4 x 4 in the row convention of `project`, in float64) of a camera at `eye` looking along (cos yaw, 0, sin yaw): t_0 and t_1 are the
    coordinates along right and up over the tangent of the half angle, t_2 = t_3 = the distance along the view direction"""
    a = np.radians(yaw_deg)
    forward, up = np.array([np.cos(a), 0.0, np.sin(a)]), np.array([0.0, 1.0, 0.0])
    right = np.cross(up, forward)
    tan_y = np.tan(np.radians(fov_deg) / 2.0)
    tan_x = tan_y * W / H
    m = np.zeros((4, 4))
    for j, axis in enumerate((right / tan_x, up / tan_y, forward, forward)):
        m[:3, j], m[3, j] = axis, -np.dot(axis, eye)
    return m


def pixel_of(m, point):
    """where the camera of `m` sees `point`, in float64: (fx, fy) of the definition's `project`"""
    t = np.append(point, 1.0) @ m
    return np.array([(t[0] / t[3] * 0.5 + 0.5) * W - OFFSET[0], (H - 1) - ((t[1] / t[3] * 0.5 + 0.5) * H - OFFSET[1])])


def reflect(point, plane_point, plane_normal):
    return point - 2.0 * np.dot(point - plane_point, plane_normal) * plane_normal


def trace_through(eye, target_image, mirrors):
    """the primary ray from `eye` towards `target_image` followed through the plane mirrors in float32, as the chain call follows it: (o, w, [d_0, d_1, ...],
    the last hit point) -- the ray's distances to each mirror in turn"""
    o = eye.astype(F)
    w = (target_image - eye)
    w = (w / np.linalg.norm(w)).astype(F)
    origin, direction, distances = o.copy(), w.copy(), []
    for plane_point, plane_normal in mirrors:
        n, q = plane_normal.astype(F), plane_point.astype(F)
        d = F(np.dot(q - origin, n) / np.dot(direction, n))
        assert d > 0
        distances.append(d)
        origin = (origin + direction * d).astype(F)
        direction = (direction - F(2.0) * F(np.dot(direction, n)) * n).astype(F)
    return o, w, distances, origin, direction


def motion_through_the_model(projected, surface_point, surface_normal, depth, chain_distance, k, prev_m):
    """the model over a uniform frame whose every pixel is the one under test, against a history that holds the same surface everywhere: (fx, fy) of pixel (7, 5),
    read back from its motion"""
    full = lambda v: np.broadcast_to(np.asarray(v, dtype=F).reshape(3, 1, 1), (3, H, W)).copy()   # noqa: E731
    ones = np.ones((H, W), dtype=F)
    colour = np.ones((H, W, 3), dtype=F)
    kk = np.full((H, W), k, dtype=np.uint32)
    history = dict(a=colour, b=colour, length=ones, depth=ones, normal=full(surface_normal), position=full(surface_point), object_id=None, chain_length=kk)
    result, motion, taken, reason, _ = chain_ref.accumulate_chain(colour, colour, ones * F(depth), full(surface_normal), full(surface_point), full(projected), kk, ones * F(chain_distance),
                                                                  history=history, prev_world_to_screen=prev_m.astype(F), prev_sample_offset=OFFSET, demodulate=False)
    assert reason[5, 7] == temporal_ref.BLENDED and taken[5, 7] >= 1
    return np.array([motion[0, 5, 7] + 7.0, motion[1, 5, 7] + 5.0], dtype=np.float64)


@pytest.mark.parametrize("mirrors", [1, 2], ids=["one_mirror", "two_facing_mirrors"])
def test_the_virtual_position_projects_to_where_the_other_camera_sees_the_reflection(mirrors):
    """A point S on a wall, seen through plane mirrors by a camera at c1: its virtual image S' is S reflected in the mirrors in reverse order.  V = o + w * D from
    c1's primary ray and the unfolded distance is S' (up to float rounding), and a second camera a small translation and yaw away sees the reflection of S
    exactly where S' projects.  1e-3 pixel is float rounding in a scene a few units across, not a tuned figure.  First-hit reprojection -- the mirror's own
    point through the second camera -- lands more than a pixel away: the test can tell the two apart."""
    ahead = (np.array([4.0, 0.0, 0.0]), np.array([-1.0, 0.0, 0.0]))    # the plane x = 4, facing the camera
    behind = (np.array([-3.0, 0.0, 0.0]), np.array([1.0, 0.0, 0.0]))   # the plane x = -3, facing the first
    planes = [ahead, behind][:mirrors]
    surface = np.array([1.5, 0.4, 2.5]) if mirrors == 1 else np.array([2.5, 0.3, 3.0])
    surface_normal = np.array([0.0, 0.0, -1.0])
    image = surface
    for plane in reversed(planes):
        image = reflect(image, *plane)
    c1, c2 = np.array([0.0, 0.5, 0.2]), np.array([0.25, 0.55, 0.1])
    m2 = pinhole(c2, 3.0 if mirrors == 1 else 4.0)
    o, w, distances, last_hit, _ = trace_through(c1, image, planes)
    last = F(np.linalg.norm(surface - last_hit.astype(np.float64)))
    total = distances[0]
    for d in distances[1:] + [last]:
        total = F(total + d)
    virtual = (o + (w * total).astype(F)).astype(F)
    assert np.abs(virtual.astype(np.float64) - image).max() < 1e-5
    want = pixel_of(m2, image)
    assert 0 < want[0] < W - 1 and 0 < want[1] < H - 1
    got = motion_through_the_model(virtual, surface, surface_normal, last, total, mirrors, m2)
    assert np.abs(got - want).max() < 1e-3, (got, want)
    # first-hit reprojection: the point on the first mirror
    first_hit = (o + w * distances[0]).astype(np.float64)
    assert np.linalg.norm(pixel_of(m2, first_hit) - want) > 1.0


# ---- 3. the rules, each on a frame built for it ----------------------------------------------------------------------------------------------------
def flat_frame(h, w):
    """a plane z = 2 facing the camera, position (x, y, 2): temporal_ref.affine_world_to_screen reprojects pixel x to x + shift"""
    ys, xs = np.mgrid[0:h, 0:w]
    normal = np.zeros((3, h, w), dtype=F)
    normal[2] = 1.0
    position = np.stack([xs, ys, np.full((h, w), 2.0)]).astype(F)
    rng = np.random.default_rng(1)
    colour = (rng.random((h, w, 3)) + 0.5).astype(F)
    return dict(color=colour, color_half=(colour * F(0.5)).astype(F), depth=np.ones((h, w), dtype=F), normal=normal, position=position)


def flat_history(h, w, k):
    f = flat_frame(h, w)
    return dict(a=f["color"], b=f["color"], length=np.full((h, w), 5.0, dtype=F), depth=f["depth"], normal=f["normal"], position=f["position"], object_id=None,
                chain_length=np.asarray(k, dtype=np.uint32))


def test_a_tap_with_another_chain_length_is_dropped():
    h, w = 9, 12
    cur = flat_frame(h, w)
    k = np.ones((h, w), dtype=np.uint32)
    prev_k = k.copy()
    prev_k[4, 6] = 2          # one history pixel seen through one mirror more
    prev_k[:, 0:2] = 0        # and a strip seen directly
    m = temporal_ref.affine_world_to_screen(w, h, (0.5, 0.5))
    args = dict(virtual_position=cur["position"], chain_length=k, chain_distance=cur["depth"], prev_world_to_screen=m, demodulate=False, **cur)
    _, _, taken, reason, _ = chain_ref.accumulate_chain(history=flat_history(h, w, prev_k), **args)
    _, _, all_taken, _, _ = chain_ref.accumulate_chain(history=flat_history(h, w, k), **args)
    assert all_taken[:h - 1, :w - 1].min() == 4
    # pixel (x, y) taps (x, y), (x + 1, y), (x, y + 1), (x + 1, y + 1): the four pixels around (6, 4) lose exactly one tap
    for y, x in ((3, 5), (3, 6), (4, 5), (4, 6)):
        assert taken[y, x] == 3 and reason[y, x] == temporal_ref.BLENDED
    assert taken[2, 2] == 4 and taken[5, 1] == 2 and taken[5, 0] == 0 and reason[5, 0] == temporal_ref.START_NO_TAP
    # the pixel's four; column 0 loses every tap (four, the last row two), column 1 the half that falls on the strip
    assert (all_taken - taken).sum() == 4 + ((h - 1) * 4 + 2) + ((h - 1) * 2 + 1)


def test_a_moments_window_straddling_the_mirrors_edge_counts_one_side_only():
    h, w = 8, 10
    f = flat_frame(h, w)
    k = np.zeros((h, w), dtype=np.uint32)
    k[:, 5:] = 1              # the mirror's edge between columns 4 and 5: same plane, same id, another chain length
    c = [np.where(k == 1, F(3.0), F(1.0)).astype(F) for _ in range(3)]
    ids = np.zeros((h, w), dtype=np.uint32)
    mu, g, cnt = chain_ref.chain_moments(c, f["depth"], f["normal"], f["position"], ids, k, 2, 1.0)
    _, _, plain = temporal_clip_ref.moments(c, f["depth"], f["normal"], f["position"], ids, 2, 1.0)
    assert plain[4, 4] == 25 and cnt[4, 4] == 15 and cnt[4, 5] == 15 and cnt[4, 3] == 20 and cnt[4, 6] == 20 and cnt[4, 7] == 25 and cnt[4, 2] == 25
    assert (mu[0][:, :5] == 1.0).all() and (mu[0][:, 5:] == 3.0).all() and not g[0].any()   # neither side's mean holds the other's colour
    # validity comes from the chain distance
    distance = f["depth"].copy()
    distance[4, 1] = np.inf
    assert chain_ref.chain_moments(c, distance, f["normal"], f["position"], ids, k, 2, 1.0)[2][4, 2] == 24


def test_with_objects_given_chain_pixels_start_and_the_others_carry_the_moving_calls_words():
    m = temporal_moving_ref.random_moving_frame(45, 23, seed=9)
    cur = m["current"]
    rng = np.random.default_rng(2)
    k = (rng.random((23, 45)) < 0.3).astype(np.uint32) * rng.integers(1, 4, size=(23, 45)).astype(np.uint32)
    virtual = (cur["position"] + F(0.25)).astype(F)   # never read: k == 0 projects P', k > 0 starts
    history = dict(m["history"], chain_length=np.zeros((23, 45), dtype=np.uint32))
    common = dict(prev_world_to_screen=m["prev_world_to_screen"], prev_sample_offset=m["prev_sample_offset"], object_motion=m["object_motion"])
    got, motion, taken, reason, _ = chain_ref.accumulate_chain(history=history, virtual_position=virtual, chain_length=k, chain_distance=cur["depth"], **cur, **common)
    want, want_motion, want_taken, want_reason = temporal_moving_ref.accumulate_moving(history=m["history"], **cur, **common)
    direct = k == 0
    assert (want_reason[~direct] == temporal_ref.BLENDED).sum() > 50 and (want_reason[direct] == temporal_ref.BLENDED).sum() > 200
    for key in ("a", "b", "length"):
        assert np.array_equal(words(got[key])[direct], words(want[key])[direct]), key
    assert np.array_equal(words(motion)[:, direct], words(want_motion)[:, direct]) and np.array_equal(taken[direct], want_taken[direct])
    start, _, _, _ = temporal_ref.accumulate(**{name: cur[name] for name in ("color", "color_half", "depth", "normal", "position", "albedo")})
    for key in ("a", "b"):
        assert np.array_equal(words(got[key])[~direct], words(start[key])[~direct]), key
    assert (got["length"][~direct] == 1.0).all() and not motion[:, ~direct].any() and not taken[~direct].any()
    assert ((reason == chain_ref.START_CHAIN_MOVED) == (~direct & (want_reason != temporal_ref.START_INVALID))).all()
    assert np.array_equal(got["chain_length"], k)


def test_the_plane_tolerance_scales_with_the_chain_distance():
    """a history plane 0.05 off the pixel's: inside 0.01 * D for D = 10, outside 0.01 * depth for the last segment's depth 1"""
    h, w = 6, 8
    cur = flat_frame(h, w)
    k = np.ones((h, w), dtype=np.uint32)
    history = flat_history(h, w, k)
    history["position"] = history["position"].copy()
    history["position"][2] += F(0.05)
    m = temporal_ref.affine_world_to_screen(w, h, (0.0, 0.0))
    args = dict(virtual_position=cur["position"], chain_length=k, history=history, prev_world_to_screen=m, demodulate=False, **cur)
    _, _, far, _, _ = chain_ref.accumulate_chain(chain_distance=np.full((h, w), 10.0, dtype=F), **args)
    _, _, near, reason, _ = chain_ref.accumulate_chain(chain_distance=cur["depth"], **args)
    assert far[2, 3] >= 1 and near[2, 3] == 0 and reason[2, 3] == temporal_ref.START_NO_TAP
    # and the call without, on the same planes, scales with depth: it drops the tap too
    plain = dict(history, chain_length=None)
    _, _, without, _, _ = temporal_clip_ref.accumulate_clip(history=plain, prev_world_to_screen=m, demodulate=False, **cur)
    assert without[2, 3] == 0


# ---- 4. two oracle recordings of the hall ----------------------------------------------------------------------------------------------------------
YAW_STEP = 0.5            # degrees between the two cameras
MAX_CHAIN = 3
# measured on the oracle's recordings (printed by the test): second-frame pixels with k >= 1, a surface guide vertex and a projection inside the frame, and
# the share of them that takes at least one tap -- over chain planes with the virtual position, and over first-hit planes fed to temporal_clip_ref
HALL_ELIGIBLE = 369
HALL_SHARE_CHAIN = 0.6748
HALL_SHARE_FIRST_HIT = 0.9973


def planes_of(frame, desc, max_chain):
    """the planes the model takes, from an oracle frame: the guide vertex's depth, normal, position and object id (zero where the reference leaves a word
    unwritten), and the chain planes"""
    import guide_chain_ref as ref
    k, distance, _, guides, stale = ref.folded_frame(frame, desc, max_chain)
    g = np.where(stale, F(0.0), guides).astype(F)
    shape = (ref.H, ref.W)
    planes = dict(depth=guides[:, 8].reshape(shape).copy(), position=g[:, 11:14].T.reshape((3,) + shape).copy(), normal=g[:, 14:17].T.reshape((3,) + shape).copy(),
                  object_id=guides[:, 6].copy().view(np.uint32).reshape(shape))
    chain = dict(virtual_position=chain_ref.virtual_frame(frame, desc, max_chain).T.reshape((3,) + shape).copy(), chain_length=k.reshape(shape), chain_distance=distance.reshape(shape))
    surface = np.array([ref.is_surface(v) for v in guides]).reshape(shape)
    return planes, chain, surface


def test_hall_reflections_find_their_history_under_a_yawing_camera(built):
    import guide_chain_ref as ref
    import oracle_lib
    import path_records_ref
    import raytracer_amd as ra
    desc = ref.scene("hall").desc
    then = ref.oracle_frame("hall")
    p_then = ref.params()
    cam = ra.Camera((-12.5, 2.5, 0.3), (-6.0, 88.0 + YAW_STEP, 0.0), ref.W / ref.H, 75.0)
    vp = ra.Viewport(ref.W, ref.H, **ref.viewport_args())
    vp.reset()
    p_now = vp.next_pass_params(cam)
    now = [oracle_lib.render_pixel_paths(desc, p_now, ref.W, ref.H, x, y, capacity=ref.MAX_RAY_DEPTH + 2) for x, y in path_records_ref.all_pixels(ref.W, ref.H)]
    colour = np.ones((ref.H, ref.W, 3), dtype=F)
    common = dict(prev_world_to_screen=np.array(p_then.camera.worldToScreen, dtype=F), prev_sample_offset=tuple(p_then.sampleOffset), demodulate=False)
    shares = {}
    eligible = None
    for label, max_chain in (("chain", MAX_CHAIN), ("first_hit", 0)):
        prev_planes, prev_chain, _ = planes_of(then, desc.contents, max_chain)
        planes, chain, surface = planes_of(now, desc.contents, max_chain)
        history = dict(prev_planes, a=colour, b=colour, length=np.ones((ref.H, ref.W), dtype=F), chain_length=prev_chain["chain_length"])
        if label == "chain":
            _, _, taken, reason, _ = chain_ref.accumulate_chain(colour, colour, history=history, **planes, **chain, **common)
            eligible = (chain["chain_length"] >= 1) & surface & np.isin(reason, (temporal_ref.BLENDED, temporal_ref.START_NO_TAP))
        else:
            _, _, taken, reason, _ = temporal_clip_ref.accumulate_clip(colour, colour, history=dict(history, chain_length=None), **planes, **common)
        shares[label] = float((taken[eligible] >= 1).mean())
    print("yaw %.2f deg, maxChain %d: %d eligible pixels; at least one tap: %.4f with chain planes, %.4f with first-hit planes" % (
        YAW_STEP, MAX_CHAIN, eligible.sum(), shares["chain"], shares["first_hit"]))
    assert shares["chain"] > 0.5
    assert int(eligible.sum()) == HALL_ELIGIBLE and round(shares["chain"], 4) == HALL_SHARE_CHAIN and round(shares["first_hit"], 4) == HALL_SHARE_FIRST_HIT
