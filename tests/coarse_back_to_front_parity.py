"""k_coarse's back-to-front form against the CPU oracle.  The oracle emits every draw; what the engine must leave of a tile's
list is the oracle's list of that tile FROM ITS LAST OPAQUE FULL COVER ONWARDS (CMD_SOLID + CMD_COLOR with alpha 255), command
words equal, CMD_FILL segment counts equal and the slices equal as multisets -- and bump.segments the sum of those lists' fill
counts, derived here from the oracle's buffers and never written down.  The scenes are tiny: small rectangles and short stroked
segments inside chosen tiles of a 128 x 128 (one quadrant of 8 x 8 tiles) or 256 x 256 (one bin, four quadrants) target, sized
by the engine's own batch size (stage_constants()["coarse_batch"]).  Shared by test_coarse_back_to_front_emu.py and
test_coarse_back_to_front_gpu.py."""
import numpy as np

from oracle.oracle import Oracle
from tests import parity
from tests.parity import BUMP_KEYS, CMD_COLOR, CMD_END, CMD_FILL, CMD_JUMP, CMD_SOLID, _CMD_SIZE

WHITE = 0xFFFFFFFF
STAGE_COARSE = 0x10
OPAQUE_FILLS_WORDS = slice(50, 58)  # engine.h Control::opaque_fills among the control block's words: any nonzero = the scene holds an opaque solid fill


# ---------------------------------------------------------------------------------------------------------------
# scenes
# ---------------------------------------------------------------------------------------------------------------
def _rect(x0, y0, x1, y1, into=None, reverse=False):
    """a closed rectangle as a path of its own, or as one more subpath of `into` (reverse: wound the other way)"""
    from vello_amd import BezPath

    p = BezPath() if into is None else into
    pts = [(x0, y0), (x1, y0), (x1, y1), (x0, y1)]
    if reverse:
        pts = [pts[0]] + pts[:0:-1]
    p.move_to((float(pts[0][0]), float(pts[0][1])))
    for x, y in pts[1:]:
        p.line_to((float(x), float(y)))
    p.close_path()
    return p


def _color(k, alpha=0.5):
    from vello_amd import Color

    return Color(0.125 * (k % 8), 0.25 * ((k // 8) % 4), 0.5 * ((k // 32) % 2), alpha)


class Builder:
    """Draws placed by tile; every coordinate is a multiple of 1/4 pixel, so areas and coverage are exact in f32."""

    def __init__(self):
        from vello_amd import Scene

        self.s = Scene()
        self.k = 0

    def small(self, tx, ty, alpha=0.5):
        """a 3 x 3 rectangle inside tile (tx, ty): segments in that tile and in no other; every 5th a short stroked segment"""
        from vello_amd import Affine, BezPath, Fill, Stroke

        k = self.k
        self.k += 1
        x, y = 16 * tx + 1 + 2.5 * (k % 5), 16 * ty + 1 + 2.5 * ((k // 5) % 5)
        if k % 5 == 4:
            p = BezPath()
            p.move_to((x, y + 1.0))
            p.line_to((x + 3.0, y + 1.0))
            self.s.stroke(Stroke(2.0), Affine.IDENTITY, _color(k, alpha), None, p)
        else:
            self.s.fill(Fill.EvenOdd if k % 3 == 0 else Fill.NonZero, Affine.IDENTITY, _color(k, alpha), None, _rect(x, y, x + 3, y + 3))

    def cover(self, tx0, ty0, tx1=None, ty1=None, brush=None, fill=None, margin=8):
        """a rectangle that covers tiles [tx0, tx1] x [ty0, ty1] fully (no segment in them) and reaches half a tile beyond"""
        from vello_amd import Affine, Color, Fill

        tx1 = tx0 if tx1 is None else tx1
        ty1 = ty0 if ty1 is None else ty1
        brush = Color(0.25, 0.5, 0.75, 1.0) if brush is None else brush
        self.k += 1
        self.s.fill(Fill.NonZero if fill is None else fill, Affine.IDENTITY, brush, None,
                    _rect(16 * tx0 - margin, 16 * ty0 - margin, 16 * (tx1 + 1) + margin, 16 * (ty1 + 1) + margin))

    def opaque_somewhere(self, tx, ty):
        """an opaque fill WITH segments in its only tile: covers nothing, but makes the scene one that holds an opaque fill"""
        self.small(tx, ty, alpha=1.0)


def cover_scene(n_beneath, n_above, witness=True):
    """tile (2, 2): n_beneath draws, an opaque cover, n_above draws; every 7th draw beneath is followed by one in the uncovered tile
    (5, 5), so the quadrant's stream holds more than the covered tile's draws"""
    b = Builder()
    for i in range(n_beneath):
        b.small(2, 2)
        if witness and i % 7 == 0:
            b.small(5, 5)
    b.cover(2, 2)
    for i in range(n_above):
        b.small(2, 2)
    return b.s, 128, 128


def cover_slot_scene(nb, first):
    """the cover as the first (slot 0) or the last (slot NB - 1) object of the batch that holds it, draws beneath in the batch before"""
    b = Builder()
    for i in range(nb // 2 + 3):
        b.small(2, 2)
    b.cover(2, 2)
    for i in range(nb - 1 if first else 0):
        b.small(2, 2 if i % 2 else 3)
    return b.s, 128, 128


def uncovered_three_batches_scene(nb, tail):
    """tile (2, 2) is never covered and its list spans three batches, the earliest of `tail` draws (5: its words fit the fixed block;
    40: they do not); tile (4, 4) gets a few draws per batch (words that fit the slack in front of a region); (6, 6) the opaque fill"""
    b = Builder()
    b.opaque_somewhere(6, 6)
    for i in range(2 * nb + tail - 1):
        b.small(2, 2)
        if i % (nb // 3) == 1:
            b.small(4, 4)
    return b.s, 128, 128


def covered_and_uncovered_scene(nb):
    """tiles (2, 2) and (5, 5) of one quadrant get the same draws, (2, 2) a cover in the middle: only its own bit may go"""
    b = Builder()
    for i in range(nb // 2 + 5):
        b.small(2, 2)
        b.small(5, 5)
    b.cover(2, 2)
    for i in range(9):
        b.small(2, 2)
        b.small(5, 5)
    return b.s, 128, 128


def all_covered_scene(nb):
    """256 x 256: more than two stream rounds of draws all over quadrant 0, then one opaque rectangle over all 64 of its tiles (its
    edge runs through the neighbouring quadrants), then a few draws on top"""
    b = Builder()
    for i in range(3 * nb + 10):
        b.small(i % 8, (i // 8) % 8)
    b.cover(0, 0, 7, 7)
    for i in range(6):
        b.small(i, 7 - i)
        b.small(9, 2 + i)
    return b.s, 256, 256


def must_not_cull_scene():
    """five tiles, each with draws beneath, something that looks like a cover and is none, and draws above"""
    from vello_amd import Affine, Color, Fill, Gradient

    b = Builder()
    tiles = [(1, 1), (3, 1), (5, 1), (1, 4), (4, 4)]
    for t in tiles:
        for i in range(6):
            b.small(*t)
    b.cover(1, 1, brush=Color.from_rgba8(10, 200, 90, 254))  # alpha 254
    b.cover(3, 1, brush=Gradient.new_linear((40.0, 8.0), (72.0, 40.0)).with_stops([(0.0, Color.from_rgba8(255, 0, 0, 255)), (1.0, Color.from_rgba8(0, 0, 255, 255))]))
    b.cover(5, 1, margin=-4)  # opaque, but its edge runs through the tile: CMD_FILL, not CMD_SOLID
    # even-odd with an even backdrop: two nested rectangles wound the same way, the tile inside both (winding 2)
    p = _rect(16 * 1 - 8, 16 * 4 - 8, 16 * 2 + 8, 16 * 5 + 8)
    _rect(16 * 1 - 4, 16 * 4 - 4, 16 * 2 + 4, 16 * 5 + 4, into=p)
    b.s.fill(Fill.EvenOdd, Affine.IDENTITY, Color(0.9, 0.1, 0.1, 1.0), None, p)
    # non-zero with backdrop 0: a frame, the tile in its hole (the inner rectangle wound the other way)
    p = _rect(16 * 4 - 8, 16 * 4 - 8, 16 * 5 + 8, 16 * 5 + 8)
    _rect(16 * 4 - 4, 16 * 4 - 4, 16 * 5 + 4, 16 * 5 + 4, into=p, reverse=True)
    b.s.fill(Fill.NonZero, Affine.IDENTITY, Color(0.1, 0.1, 0.9, 1.0), None, p)
    for t in tiles:
        for i in range(3):
            b.small(*t)
    return b.s, 128, 128


def clip_pair_scene(nb):
    """one clip pair: the forward form, whatever covers the scene holds"""
    from vello_amd import Affine, BlendMode, Compose, Fill, Mix, Rect

    b = Builder()
    for i in range(nb // 2):
        b.small(2, 2)
    b.cover(2, 2)
    b.s.push_layer(Fill.NonZero, BlendMode(Mix.Normal, Compose.SrcOver), 1.0, Affine.IDENTITY, Rect(20.0, 20.0, 90.0, 90.0))
    for i in range(12):
        b.small(2 + i % 3, 2)
    b.s.pop_layer()
    for i in range(4):
        b.small(2, 2)
    return b.s, 128, 128


def no_opaque_scene(nb):
    """nothing opaque: alpha-254 covers and translucent draws only"""
    from vello_amd import Color

    b = Builder()
    for i in range(nb + 20):
        b.small(2, 2)
        if i % 50 == 0:
            b.cover(2, 2, brush=Color.from_rgba8(10, 200, 90, 254))
    return b.s, 128, 128


def random_cover_scene(n_paths, size, seed=5):
    """the counter's derivation at a size between the tiny scenes and d2: opaque rectangles of a few tiles among many small draws"""
    from vello_amd import Affine, Color, Fill, Scene

    rng = np.random.default_rng(seed)
    s = Scene()
    for k in range(n_paths):
        x, y = rng.uniform(0, size, 2)
        if k % 40 == 39:
            w, h = rng.uniform(30, 90, 2)
            s.fill(Fill.NonZero, Affine.IDENTITY, Color(float(rng.uniform(0, 1)), float(rng.uniform(0, 1)), 0.5, 1.0), None, _rect(x, y, x + w, y + h))
        else:
            w, h = rng.uniform(2, 14, 2)
            s.fill(Fill.EvenOdd if k % 2 else Fill.NonZero, Affine.IDENTITY, Color(float(rng.uniform(0, 1)), 0.5, float(rng.uniform(0, 1)), float(rng.uniform(0.3, 1.0))), None,
                   _rect(x, y, x + w, y + h))
    return s, size, size


# ---------------------------------------------------------------------------------------------------------------
# lists
# ---------------------------------------------------------------------------------------------------------------
def walk_lists(name, ptcl, n_tiles):
    """per tile: its commands as (word index, tag) in list order, jumps followed and left out"""
    out = []
    for t in range(n_tiles):
        ix, cmds = t * 64 + 1, []
        for _ in range(1 << 20):
            assert ix < ptcl.size, f"{name}: tile {t}: the list leaves the pool"
            tag = int(ptcl[ix])
            if tag == CMD_JUMP:
                ix = int(ptcl[ix + 1])
                continue
            if tag == CMD_END:
                break
            assert tag < 16 and _CMD_SIZE[tag] > 0, f"{name}: tile {t}: unknown PTCL command {tag} at word {ix}"
            cmds.append((ix, tag))
            ix += int(_CMD_SIZE[tag])
        else:
            raise AssertionError(f"{name}: tile {t}: the list does not end")
        out.append(cmds)
    return out


def from_last_cover(ptcl, cmds):
    """the commands from the tile's last opaque full cover onwards: CMD_SOLID followed by CMD_COLOR with alpha 255"""
    start = 0
    for i in range(len(cmds) - 1):
        if cmds[i][1] == CMD_SOLID and cmds[i + 1][1] == CMD_COLOR and (int(ptcl[cmds[i + 1][0] + 1]) >> 24) == 0xFF:
            start = i
    return cmds[start:]


def compare_lists(name, engine, oracle, n_tiles, bump, cull=True):
    """The engine's lists against the oracle's from the last cover onwards (cull=False: against the whole lists).  Returns the number
    of segments the expected lists' fills hold, and how many commands the covers hide."""
    ptcl_o = oracle.buffer("ptcl", np.uint32)[: 64 * n_tiles + oracle.bump()["ptcl"]]
    ptcl_h = engine.read_buffer("ptcl", np.uint32, (64 * n_tiles + bump["ptcl"]) * 4)
    lo, lh = walk_lists(name + " (oracle)", ptcl_o, n_tiles), walk_lists(name, ptcl_h, n_tiles)
    fh, fo, fn = [], [], []
    hidden = 0
    for t in range(n_tiles):
        want = from_last_cover(ptcl_o, lo[t]) if cull else lo[t]
        hidden += len(lo[t]) - len(want)
        got = lh[t]
        assert [c[1] for c in got] == [c[1] for c in want], \
            f"{name}: tile {t}: commands {[c[1] for c in got][:24]} ({len(got)}), expected {[c[1] for c in want][:24]} ({len(want)} of the oracle's {len(lo[t])})"
        for (ih, tag), (io, _) in zip(got, want):
            n = int(_CMD_SIZE[tag])
            wh, wo = ptcl_h[ih: ih + n].copy(), ptcl_o[io: io + n].copy()
            if tag == CMD_FILL:  # word 2 is the slice's place: allocation order
                fh.append(int(wh[2]))
                fo.append(int(wo[2]))
                fn.append(int(wo[1]) >> 1)
                wh[2] = wo[2] = 0
            assert np.array_equal(wh, wo), f"{name}: tile {t}: command {tag} at word {ih}: {wh} expected {wo}"
        assert int(ptcl_h[t * 64 + 63]) == sum(int(_CMD_SIZE[c[1]]) for c in got), f"{name}: tile {t}: the list's length word"
    fh, fo, fn = (np.array(x, dtype=np.int64) for x in (fh, fo, fn))
    total = int(fn.sum())
    if total:
        assert int(fh.max()) + int(fn[np.argmax(fh)]) <= bump["segments"], f"{name}: a fill's slice lies beyond bump.segments"
        # the slices the engine handed out are disjoint and fill [0, bump.segments)
        order = np.argsort(fh)
        assert np.array_equal(fh[order], np.cumsum(fn[order]) - fn[order]), f"{name}: the fills' slices overlap or leave holes"
        parity.compare_segment_slices(name, engine.read_buffer("segments", np.uint32, bump["segments"] * 24),
                                      oracle.buffer("segments", np.uint32)[: oracle.bump()["segments"] * 6], fh, fo, fn)
    return total, hidden


def resolve(scene):
    import vello_amd

    return vello_amd.Resolver().resolve(scene)


def check_scene(engine, scene, w, h, name, back_to_front=True, min_hidden=1, aas=None):
    """Image (both AA modes, against the oracle and the no_cull twin), list and counter of one scene.  back_to_front: the form the
    scene must take.  min_hidden: commands the covers must hide (0: the scene has none to hide)."""
    from vello_amd import AaConfig

    r = resolve(scene)
    n_tiles = ((w + 15) // 16) * ((h + 15) // 16)
    oracle = Oracle(capacity_scale=4)
    out = {}
    for aa in aas or (AaConfig.Area, AaConfig.Msaa16):
        tag = f"{name}_{int(aa)}"
        oracle.set_scene(r.packed, r.layout, w, h, WHITE, int(aa))
        oracle.set_ramps(r.ramps)
        ref = oracle.render()
        ob = oracle.bump()
        assert ob["failed"] == 0, f"{tag}: the oracle's pools overflow: {ob}"
        img, bump = engine.render(r.packed, r.layout, w, h, WHITE, aa, ramps=r.ramps)
        img = img.copy()
        assert bump["failed"] == 0, f"{tag}: {bump}"
        took = bool(engine.control_words()[OPAQUE_FILLS_WORDS].any()) and r.layout.n_clips == 0
        assert took == back_to_front, f"{tag}: the scene takes the {'back-to-front' if took else 'forward'} form"
        assert all(bump[k] == ob[k] for k in BUMP_KEYS if k not in ("segments", "ptcl")), f"{tag}: counters ahead of coarse differ: hip {bump} oracle {ob}"
        if r.layout.n_clips == 0:
            want_segments, hidden = compare_lists(tag, engine, oracle, n_tiles, bump, cull=True)
            print(f"{tag}: bump.segments {bump['segments']} (oracle {ob['segments']}, from the last covers {want_segments}), bump.ptcl {bump['ptcl']}, hidden commands {hidden}")
            assert hidden >= min_hidden, f"{tag}: the covers hide {hidden} commands: the case does not exercise culling"
            assert bump["segments"] == want_segments, f"{tag}: bump.segments {bump['segments']}, the lists from the last covers hold {want_segments}"
        engine.update_debug_flags(no_cull=True)
        try:
            twin, b2 = engine.render(r.packed, r.layout, w, h, WHITE, aa, ramps=r.ramps)
            assert all(b2[k] == ob[k] for k in BUMP_KEYS if k != "ptcl"), f"{tag}: counters differ with no_cull: hip {b2} oracle {ob}"
            n_all, _ = compare_lists(tag + "_nocull", engine, oracle, n_tiles, b2, cull=False)
            assert n_all == ob["segments"]
        finally:
            engine.update_debug_flags(no_cull=False)
        print(f"{tag}: image max |engine - oracle| {np.abs(img.astype(int) - ref.astype(int)).max()}, max |engine - twin| {np.abs(img.astype(int) - twin.astype(int)).max()}")
        assert np.array_equal(img, twin), f"{tag}: image differs from the no_cull twin"
        assert np.array_equal(img, ref), f"{tag}: image differs from the oracle's"
        out[int(aa)] = (bump, b2)
    return out


# ---------------------------------------------------------------------------------------------------------------
# the cases, shared by the emulated and the GPU suite
# ---------------------------------------------------------------------------------------------------------------
def batch(engine):
    return engine.stage_constants()["coarse_batch"]


def check_cover_boundaries(engine, name, which, n_above):
    nb = batch(engine)
    n = {"nb-1": nb - 1, "nb": nb, "nb+1": nb + 1, "2nb+1": 2 * nb + 1}[which]
    s, w, h = cover_scene(n, n_above)
    check_scene(engine, s, w, h, f"{name}_{which}_{n_above}", min_hidden=n)


def check_cover_slot(engine, name, first):
    s, w, h = cover_slot_scene(batch(engine), first)
    check_scene(engine, s, w, h, f"{name}_{'first' if first else 'last'}", min_hidden=batch(engine) // 2)


def check_uncovered_three_batches(engine, name, tail):
    nb = batch(engine)
    s, w, h = uncovered_three_batches_scene(nb, tail)
    res = check_scene(engine, s, w, h, f"{name}_{tail}", min_hidden=0)
    for bump, twin in res.values():
        assert bump["segments"] == twin["segments"], f"{name}: nothing is covered, yet bump.segments {bump['segments']} != {twin['segments']}"
    # the shape of tile (2, 2)'s storage: a jump chain over three batches; its fixed block holds the earliest batch's commands when they
    # fit (tail * 6 words <= 60) and a lone jump when they do not
    from vello_amd import AaConfig

    r = resolve(s)
    engine.render(r.packed, r.layout, w, h, WHITE, AaConfig.Msaa16)  # (check_scene's last frame was the no_cull twin)
    ptcl = engine.read_buffer("ptcl", np.uint32)
    t = 2 * 8 + 2
    first = int(ptcl[t * 64 + 1])
    assert (first != CMD_JUMP) == (tail * 6 <= 60), f"{name}: tile (2, 2)'s fixed block starts with command {first}"
    jumps, ix = 0, t * 64 + 1
    while int(ptcl[ix]) != CMD_END:
        tag = int(ptcl[ix])
        if tag == CMD_JUMP:
            jumps += 1
            ix = int(ptcl[ix + 1])
        else:
            ix += int(_CMD_SIZE[tag])
    assert 2 <= jumps <= 3, f"{name}: tile (2, 2)'s list takes {jumps} jumps over three batches"
    # tile (4, 4): a few draws per batch: the later batches' words went in front of the first region's, in place: ONE jump (out of the fixed block)
    jumps, ix = 0, (4 * 8 + 4) * 64 + 1
    while int(ptcl[ix]) != CMD_END:
        tag = int(ptcl[ix])
        if tag == CMD_JUMP:
            jumps += 1
            ix = int(ptcl[ix + 1])
        else:
            ix += int(_CMD_SIZE[tag])
    assert jumps == 1, f"{name}: tile (4, 4)'s list takes {jumps} jumps: its batches' words were not prepended in place"


def check_covered_and_uncovered(engine, name):
    s, w, h = covered_and_uncovered_scene(batch(engine))
    check_scene(engine, s, w, h, name, min_hidden=batch(engine) // 2)


def check_all_covered(engine, name):
    nb = batch(engine)
    s, w, h = all_covered_scene(nb)
    check_scene(engine, s, w, h, name, min_hidden=3 * nb)


def check_must_not_cull(engine, name):
    s, w, h = must_not_cull_scene()
    res = check_scene(engine, s, w, h, name, min_hidden=0)
    for bump, twin in res.values():
        assert bump["segments"] == twin["segments"], f"{name}: something was culled: bump.segments {bump['segments']}, no_cull {twin['segments']}"


def check_clip_pair(engine, name):
    """forward form: word-exact buffers with no_cull through the existing helpers, the image in default mode"""
    from vello_amd import AaConfig

    s, w, h = clip_pair_scene(batch(engine))
    r = resolve(s)
    assert r.layout.n_clips == 2
    for aa in (AaConfig.Area, AaConfig.Msaa16):
        parity.compare_frame(engine, r.packed, r.layout, w, h, WHITE, aa, f"{name}_{int(aa)}", tol=0, resolved=r)
    check_scene(engine, s, w, h, name, back_to_front=False)


def check_no_opaque(engine, name):
    s, w, h = no_opaque_scene(batch(engine))
    res = check_scene(engine, s, w, h, name, back_to_front=False, min_hidden=0)
    for bump, twin in res.values():
        assert bump["ptcl"] == twin["ptcl"] and bump["segments"] == twin["segments"], f"{name}: default {bump}, no_cull {twin}"


def check_ptcl_pool_short(make_engine, name):
    """A PTCL pool one word short of the frame's demand: the last region does not fit.  The frame reports STAGE_COARSE and its whole
    demand; with the pool grown by it the frame is correct."""
    from vello_amd import AaConfig

    probe = make_engine(None)
    nb = batch(probe)
    s, w, h = uncovered_three_batches_scene(nb, 40)
    r = resolve(s)
    n_tiles = ((w + 15) // 16) * ((h + 15) // 16)
    _, good = probe.render(r.packed, r.layout, w, h, WHITE, AaConfig.Msaa16)
    assert good["failed"] == 0 and good["ptcl"] > 0
    eng = make_engine({"ptcl": 64 * n_tiles + good["ptcl"] - 1})
    assert eng.capacities()["ptcl"] == 64 * n_tiles + good["ptcl"] - 1
    _, bump = eng.render(r.packed, r.layout, w, h, WHITE, AaConfig.Msaa16)
    print(f"{name}: demand {good['ptcl']}, with the pool one word short: {bump}")
    assert bump["failed"] & STAGE_COARSE, f"{name}: {bump}"
    assert bump["ptcl"] == good["ptcl"] and bump["segments"] == good["segments"], f"{name}: the demand left behind: {bump}, the frame's {good}"
    assert eng.sync() == -4
    assert eng.grow_pools(bump)
    check_scene(eng, s, w, h, name + "_grown", min_hidden=0, aas=(AaConfig.Msaa16,))


def check_in_flight(engine, name, n):
    """n frames in flight of a resident scene: every frame's image and counters are the blocking frame's"""
    from vello_amd import AaConfig

    nb = batch(engine)
    s, w, h = cover_scene(nb + 1, 10)
    r = resolve(s)
    ref, bump = engine.render(r.packed, r.layout, w, h, WHITE, AaConfig.Msaa16)
    ref = ref.copy()
    try:
        engine.upload_scene(r.packed, r.layout)
        engine.set_frames_in_flight(n)
        for k in range(2 * n):
            engine.render_resident(w, h, WHITE, AaConfig.Msaa16)
        for k in range(n):
            engine.render_resident(w, h, WHITE, AaConfig.Msaa16)
            engine.sync_frame(0)
            b = engine.bump()
            assert b == bump, f"{name}: frame {k}: {b}, blocking {bump}"
            assert np.array_equal(engine.read_buffer("output", np.uint8, w * h * 4).reshape(h, w, 4), ref), f"{name}: frame {k}: image"
        assert engine.sync() == 0
    finally:
        engine.set_frames_in_flight(1)


def check_front_ends(engine, name):
    """a resident scene through the indexed and the unindexed front end: the same lists either way"""
    from vello_amd import AaConfig

    nb = batch(engine)
    s, w, h = cover_scene(nb + 1, 10)
    r = resolve(s)
    ref, bump = engine.render(r.packed, r.layout, w, h, WHITE, AaConfig.Msaa16)
    ref = ref.copy()
    oracle = Oracle(capacity_scale=4)
    oracle.set_scene(r.packed, r.layout, w, h, WHITE, int(AaConfig.Msaa16))
    oracle.render()
    engine.upload_scene(r.packed, r.layout)
    try:
        for unindexed in (False, True):
            engine.set_debug_flags(no_scene_index=unindexed)
            engine.render_resident(w, h, WHITE, AaConfig.Msaa16)
            engine.sync_frame(0)
            b = engine.bump()
            assert b == bump, f"{name}: unindexed={unindexed}: {b}, blocking {bump}"
            n_seg, hidden = compare_lists(f"{name}_{int(unindexed)}", engine, oracle, 64, b)
            assert n_seg == b["segments"] and hidden >= nb
            assert np.array_equal(engine.read_buffer("output", np.uint8, w * h * 4).reshape(h, w, 4), ref), f"{name}: unindexed={unindexed}: image"
    finally:
        engine.set_debug_flags()


def expected_segments(oracle, n_tiles):
    """bump.segments of a frame whose lists start at their last covers, from the oracle's PTCL alone (vectorised: d2 has 10 000 tiles
    and a million commands).  Walks all tiles in lockstep; a cover resets its tile's sum."""
    ptcl = oracle.buffer("ptcl", np.uint32)[: 64 * n_tiles + oracle.bump()["ptcl"]].astype(np.int64)
    ix = np.arange(n_tiles, dtype=np.int64) * 64 + 1
    total = np.zeros(n_tiles, dtype=np.int64)
    after_solid = np.zeros(n_tiles, dtype=bool)
    active = np.arange(n_tiles)
    for _ in range(1 << 22):
        if active.size == 0:
            break
        i = ix[active]
        tag = ptcl[i]
        j = tag == CMD_JUMP
        if j.any():
            ix[active[j]] = ptcl[i[j] + 1]
            continue
        f = tag == CMD_FILL
        total[active[f]] += ptcl[i[f] + 1] >> 1
        # a cover is CMD_SOLID and the CMD_COLOR behind it (the oracle's chunks may put a jump between the two)
        cov = (tag == CMD_COLOR) & after_solid[active] & ((ptcl[np.minimum(i + 1, ptcl.size - 1)] >> 24) == 0xFF)
        total[active[cov]] = 0
        after_solid[active] = tag == CMD_SOLID
        ix[active] += _CMD_SIZE[tag]
        active = active[tag != CMD_END]
    else:
        raise AssertionError("PTCL walk did not terminate")
    return int(total.sum())


def check_counter_large(engine, packed, layout, w, h, aa, name, oracle):
    """failed == 0, the image equal to the no_cull twin's, bump.segments strictly below the twin's and equal to what the oracle's lists
    hold from their last covers onwards"""
    oracle.set_scene(packed, layout, w, h, WHITE, int(aa))
    oracle.render()
    ob = oracle.bump()
    assert ob["failed"] == 0, ob
    n_tiles = ((w + 15) // 16) * ((h + 15) // 16)
    want = expected_segments(oracle, n_tiles)
    img, bump = engine.render(packed, layout, w, h, WHITE, aa)
    img = img.copy()
    engine.update_debug_flags(no_cull=True)
    try:
        twin, b2 = engine.render(packed, layout, w, h, WHITE, aa)
    finally:
        engine.update_debug_flags(no_cull=False)
    print(f"{name}: bump.segments {bump['segments']}, no_cull {b2['segments']}, the oracle's lists from their last covers {want}; bump.ptcl {bump['ptcl']} / {b2['ptcl']}")
    assert bump["failed"] == 0 and b2["failed"] == 0, f"{name}: {bump} {b2}"
    assert b2["segments"] == ob["segments"]
    assert np.array_equal(img, twin), f"{name}: image differs from the no_cull twin"
    assert bump["segments"] < b2["segments"], f"{name}: bump.segments {bump['segments']}, no_cull {b2['segments']}"
    assert bump["segments"] == want, f"{name}: bump.segments {bump['segments']}, expected {want}"
    return bump, b2
