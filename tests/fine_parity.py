"""k_fine at the edges of its batch planner, command windows and slice cuts.  Every size comes from Engine.stage_constants().

The generators stack draws in tile (0, 0) of a target of one to four tiles, with control over the FILLs of the tile's list, the
words between them and every fill's segments, crossing records and rule.  plan_tile() is the tests' own statement of what k_fine
must do with a command list (the comments at ms_build_batch and at the MSAA arm of k_fine, restated): it reads the PTCL words and
the segments the ENGINE wrote for the frame and returns the windows, the fills each window shows, the fills kept after the segment,
fill and record limits, the regular prefix and the path every fill takes.  Every case asserts through it that the edge it is named
after was hit in the frame under test, and only then compares the frame with the oracle through parity.compare_frame (MSAA
bit-exact, area AA within 1 plus the exact same-order check, all stages, the back half).

What coarse can write bounds what a window can show: a path draw is FILL or SOLID plus a draw command of two or three words, a
BEGIN_CLIP is one word, an END_CLIP comes with its clip path's FILL or SOLID in front.  Two FILLs are therefore at least six words
apart and a window of 64 words shows at most eleven of them: fine_batch_fills (12) is out of reach of any list coarse writes, which
check_densest_window states as an assertion.

Shared by tests/test_fine_shapes_emu.py (the SIMT-emulated build) and tests/test_fine_shapes_gpu.py (the MI355X)."""
import numpy as np

from oracle.oracle import Oracle
from tests.parity import _CMD_SIZE, CMD_COLOR, CMD_END, CMD_FILL, CMD_JUMP, CMD_SOLID, compare_frame

BLACK = 0xFF000000
TILE = 16


def make_oracle():
    return Oracle(capacity_scale=4, auto_grow=True)


def colour(k, alpha=120):
    from vello_amd import Color

    return Color.from_rgba8(30 + (k * 37) % 220, 250 - (k * 53) % 220, 40 + (k * 91) % 200, alpha)


# ---------------------------------------------------------------------------------------------------------------
# The planner model
# ---------------------------------------------------------------------------------------------------------------
def _span(a, b):
    return int(max(np.ceil(max(a, b)) - np.floor(min(a, b)), np.float32(1.0)))


def crossings(p0x, p0y, p1x, p1y):
    """Crossing records of one segment (fine.wgsl:186-215): span(x) + span(y) - 1, none for a horizontal segment on an integer row."""
    p0x, p0y, p1x, p1y = (np.float32(v) for v in (p0x, p0y, p1x, p1y))
    if p0y == p1y and p0y == np.floor(p0y):
        return 0
    return _span(p0x, p1x) + _span(p0y, p1y) - 1


def fill_records(segments, seg_ix, n_segs):
    s = segments.reshape(-1, 6)[seg_ix: seg_ix + n_segs]
    assert len(s) == n_segs, "a FILL's segments leave the buffer"
    return sum(crossings(*r[:4]) for r in s)


class Batch:
    """One call of the batch planner: `base` the window's first word, `how` the window was come by ("fresh": loaded at the FILL;
    "reused": the window requested when the previous batch was staged; "same": the interpreter's window already began at the FILL),
    `shown` the window offsets of the FILLs the window shows, `kept` how many of them stay after the segment and fill limits, `fit`
    after the record limit as well (0: the first fill goes unbatched), `ends` the record ranges' ends of the kept fills, `fast` the
    length of the regular prefix, `cut` the fills of the prefix a slice's end took away."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def __repr__(self):
        return f"Batch({self.__dict__})"


def plan_tile(ptcl, segments, tile_ix, c, fill_lo=0, fill_hi=None):
    """What k_fine's MSAA arm does with tile `tile_ix`'s list: (batches, fills, total FILLs of the walk).  fills: per FILL taken a
    dict -- no (its number in the list), at (its word), off (its offset in the window of its batch), segs, records, even_odd, path
    ("simple", "batch", "unbatched"), batch (index into batches).  fill_lo / fill_hi: the walk of the slice that owns the fills
    [fill_lo, fill_hi) (it passes over the FILLs in front and ends behind its last)."""
    W, reach = c["fine_window_words"], c["fine_prefetch_reach"]
    sliced = fill_hi is not None or fill_lo != 0
    hi = fill_hi if fill_hi is not None else 1 << 62

    def word(a):
        return int(ptcl[a]) if a < len(ptcl) else 0

    cmd = tile_ix * c["ptcl_initial_alloc"]
    win_base = cmd
    cmd += 1
    pf_base = None
    staged = []  # the staged fills not yet replayed
    fast_left, fast_after = 0, 0
    clean = False
    fill_no = 0
    batches, fills = [], []

    def scan(base, at):
        """The window at `base`, read from the FILL at `at` on."""
        chain = []  # (offset, tag) of the commands the walk reaches
        p = at - base
        while True:
            tag = word(base + p)
            chain.append((p, tag))
            size = int(_CMD_SIZE[tag]) if tag < 16 else 0
            if size == 0 or p > W - 4 or p + size >= W:  # END, JUMP; no FILL fits behind here; the next command begins outside
                break
            p += size
        shown = [(k, p) for k, (p, tag) in enumerate(chain) if tag == CMD_FILL and p <= W - 4]
        info = []
        for k, p in shown:
            rule_n = word(base + p + 1)
            info.append({"k": k, "off": p, "segs": rule_n >> 1, "even_odd": rule_n & 1, "seg_ix": word(base + p + 2)})
        kept, total = 0, 0
        for f in info:  # the batch ends in front of the first FILL whose segments no longer fit, and after fine_batch_fills fills
            total += f["segs"]
            if total > c["fine_batch_segments"] or kept == c["fine_batch_fills"]:
                break
            kept += 1
        b = Batch(base=base, s0=at - base, shown=[f["off"] for f in info], kept=kept, fit=0, ends=[], fast=0, cut=0, after=None,
                  segs=[f["segs"] for f in info], prefetch=None, simple=[])
        if kept == 0:
            return b, []
        b.prefetch = base + info[kept - 1]["off"] + 4
        end = 0
        for f in info[:kept]:
            f["records"] = fill_records(segments, f["seg_ix"], f["segs"])
            end += f["records"]
            b.ends.append(end)
        b.fit = sum(1 for e in b.ends if e <= c["fine_item_cap"])
        assert all(e <= c["fine_item_cap"] for e in b.ends[: b.fit])
        # the regular prefix: kept FILL, COLOR wholly inside the window, kept FILL, ...
        kept_k = {f["k"] for f in info[:kept]}
        pairs = 0
        while (2 * pairs in kept_k and 2 * pairs + 1 < len(chain) and chain[2 * pairs + 1][1] == CMD_COLOR
               and chain[2 * pairs + 1][0] <= W - 2 and info[pairs]["k"] == 2 * pairs):
            pairs += 1
        b.fast = min(b.fit, pairs)
        if b.fast:
            b.after = base + chain[2 * b.fast - 1][0] + 2
        b.simple = [f["even_odd"] == 0 and 1 <= f["records"] <= c["fine_simple_records"] for f in info[: b.fit]]
        return b, info[: b.fit]

    def take(f, path):
        nonlocal fill_no
        fills.append({"no": fill_no, "at": f["at"], "off": f["off"], "segs": f["segs"], "records": f.get("records"), "even_odd": f["even_odd"],
                      "path": path, "batch": len(batches) - 1})
        fill_no += 1

    for _ in range(1 << 20):
        if cmd + 4 > win_base + W:
            win_base = cmd
        tag = word(cmd)
        if tag == CMD_END:
            break
        if tag == CMD_FILL:
            if fill_no < fill_lo:
                fill_no += 1
                cmd += 4
                continue
            if not staged:
                how = "same"
                if cmd != win_base:
                    if pf_base is not None and pf_base <= cmd <= pf_base + reach:
                        win_base, how = pf_base, "reused"
                    else:
                        win_base, how = cmd, "fresh"
                b, staged = scan(win_base, cmd)
                b.how = how
                batches.append(b)
                for f in staged:
                    f["at"] = win_base + f["off"]
                pf_base = b.prefetch
                fast_left, fast_after = b.fast, b.after
                if sliced and fast_left > hi - fill_no:  # the slice ends inside the regular prefix
                    b.cut = fast_left - (hi - fill_no)
                    fast_left = hi - fill_no
            if staged:
                if fast_left:
                    for _ in range(fast_left):
                        f = staged.pop(0)
                        slot = len(batches[-1].simple) - len(staged) - 1
                        if clean and batches[-1].simple[slot]:
                            take(f, "simple")
                        else:
                            take(f, "batch")
                            clean = not f["even_odd"]
                    fast_left = 0
                    if sliced and fill_no >= hi:
                        break
                    cmd = fast_after
                    continue
                f = staged.pop(0)
                assert f["at"] == cmd, "the interpreter reached a FILL that is not the batch's next"
                take(f, "batch")
                clean = not f["even_odd"]
            else:
                rule_n = word(cmd + 1)
                b = batches[-1]
                take({"at": cmd, "off": cmd - win_base, "segs": rule_n >> 1, "even_odd": rule_n & 1,
                      "records": fill_records(segments, word(cmd + 2), rule_n >> 1)}, "unbatched")
                clean = False
            cmd += 4
            if sliced:
                if fill_no >= hi:
                    break
                continue
            if cmd + 2 <= win_base + W and word(cmd) == CMD_COLOR:
                cmd += 2
        elif tag == CMD_JUMP:
            cmd = word(cmd + 1)
        elif tag == CMD_SOLID and not sliced:
            cmd += 1
            if cmd + 2 <= win_base + W and word(cmd) == CMD_COLOR:
                cmd += 2
        else:
            size = int(_CMD_SIZE[tag]) if tag < 16 else 0
            assert size > 0, f"unknown PTCL command {tag} at {cmd}"
            cmd += size
    else:
        raise AssertionError("the walk did not end")
    return batches, fills, fill_no


def list_words(ptcl, tile_ix, c):
    """The tile's commands in order, CMD_JUMPs followed: [(tag, word index)]; and the list's length as coarse left it for fine."""
    out = []
    cmd = tile_ix * c["ptcl_initial_alloc"] + 1
    for _ in range(1 << 20):
        tag = int(ptcl[cmd])
        out.append((tag, cmd))
        if tag == CMD_END:
            break
        cmd = int(ptcl[cmd + 1]) if tag == CMD_JUMP else cmd + int(_CMD_SIZE[tag])
    return out, int(ptcl[(tile_ix + 1) * c["ptcl_initial_alloc"] - 1])


def plan_area(ptcl, tile_ix, c):
    """The area-AA arm's look-ahead: per FILL (its offset in the interpreter's window, segments, what it requests ahead: None, or
    the (offset, segments, seg_data) of the next FILL -- behind an optional COLOR and wholly inside the window)."""
    W = c["fine_window_words"]
    cmd = tile_ix * c["ptcl_initial_alloc"]
    win_base = cmd
    cmd += 1
    out = []
    for _ in range(1 << 20):
        if cmd + 4 > win_base + W:
            win_base = cmd
        tag = int(ptcl[cmd])
        if tag == CMD_END:
            break
        if tag == CMD_FILL:
            nx = cmd + 4
            if nx + 2 <= win_base + W and ptcl[nx] == CMD_COLOR:
                nx += 2
            ahead = None
            if nx + 4 <= win_base + W and ptcl[nx] == CMD_FILL:
                ahead = (nx - win_base, int(ptcl[nx + 1]) >> 1, int(ptcl[nx + 2]))
            out.append({"off": cmd - win_base, "segs": int(ptcl[cmd + 1]) >> 1, "seg_ix": int(ptcl[cmd + 2]), "ahead": ahead,
                        "next_fill_off": nx - win_base if ptcl[nx] == CMD_FILL else None})
            cmd += 4
            if cmd + 2 <= win_base + W and ptcl[cmd] == CMD_COLOR:
                cmd += 2
        elif tag == CMD_JUMP:
            cmd = int(ptcl[cmd + 1])
        elif tag == CMD_SOLID:
            cmd += 1
            if cmd + 2 <= win_base + W and ptcl[cmd] == CMD_COLOR:
                cmd += 2
        else:
            cmd += int(_CMD_SIZE[tag])
    return out


# ---------------------------------------------------------------------------------------------------------------
# Generators: contours inside tile (0, 0), lists of draws
# ---------------------------------------------------------------------------------------------------------------
def rect_c(cols, rows, k=0, x=1, y=1):
    """A rectangle over cols x rows pixels: 4 segments, 2 (cols + rows) records."""
    x0, y0 = x + 0.2 + 0.03 * (k % 10), y + 0.2 + 0.03 * ((k // 10) % 10)
    x1, y1 = x0 + cols - 0.6, y0 + rows - 0.6
    return [(x0, y0), (x1, y0), (x1, y1), (x0, y1)]


def tri_c(cols, rows, k=0, x=1, y=1):
    """A right triangle over cols x rows pixels: 3 segments, 2 (cols + rows) - 1 records."""
    r = rect_c(cols, rows, k, x, y)
    return [r[0], r[1], r[2]]


def ngon_c(n, k=0, radius=5.5):
    """A regular n-gon round (8, 8): n short segments."""
    a = 2.0 * np.pi * (np.arange(n) + 0.13 * (k % 7)) / n
    return [(8.0 + radius * np.cos(t), 8.1 + radius * np.sin(t)) for t in a]


def tall_c(n, k=0):
    """n long diagonals from the tile's top to its bottom and back: about 15 records a segment."""
    xs = 0.63 + 14.6 * np.arange(n) / (n - 1) + 0.01 * (k % 10)
    return [(float(x), 0.6 if i % 2 == 0 else 15.4) for i, x in enumerate(xs)]


def host_counts(contours):
    """(segments, records) of closed contours that lie inside tile (0, 0), by the model's crossing rule."""
    segs = recs = 0
    for pts in contours:
        for i in range(len(pts)):
            a, b = pts[i], pts[(i + 1) % len(pts)]
            segs += 1
            recs += crossings(a[0], a[1], b[0], b[1])
    return segs, recs


def exact_c(records, k=0):
    """Contours of exactly `records` crossing records (>= 3): rectangles of 40 and one rectangle or triangle for the rest."""
    out = []
    i = 0
    while records > 56:
        out.append(rect_c(10, 10, k + i, x=1 + i % 3, y=1 + (i // 3) % 3))
        records -= 40
        i += 1
    assert records >= 3
    half = (records + 1) // 2  # cols + rows
    cols = min(14, half - 1)
    out.append(rect_c(cols, half - cols, k + i) if records % 2 == 0 else tri_c(cols, half - cols, k + i))
    return out


def tuned_c(records, n_tall, k=0):
    """tall_c(n_tall) brought to exactly `records` records by exact_c's contours."""
    t = [tall_c(n_tall, k)]
    return t + exact_c(records - host_counts(t)[1], k)


class TileList:
    """A scene whose draws all touch tile (0, 0), and what its list must hold: `expect` is (segments, records, even_odd) per FILL of
    the tile's list in list order (records None where the contours leave the tile)."""

    def __init__(self, w=TILE, h=TILE):
        from vello_amd import Scene

        self.s, self.w, self.h, self.k = Scene(), w, h, 0
        self.expect, self.open, self.words, self.brushes = [], [], 0, False

    def _path(self, contours):
        from vello_amd import BezPath

        p = BezPath()
        for pts in contours:
            p.move_to(pts[0])
            for q in pts[1:]:
                p.line_to(q)
            p.close_path()
        return p

    def _cover(self):
        from vello_amd import Rect

        return Rect(-3.0, -3.0, self.w + 3.0, self.h + 3.0)

    def fill(self, contours, even_odd=False, gradient=False, records=True, alpha=120):
        """FILL + COLOR (6 words); gradient: FILL + LIN_GRAD (7)."""
        from vello_amd import Affine, Fill, Gradient

        brush = colour(self.k, alpha)
        if gradient:
            brush = Gradient.new_linear((0.0, 0.0), (16.0, 12.0)).with_stops([colour(self.k, 90), colour(self.k + 5, 200)])
            self.brushes = True
        self.s.fill(Fill.EvenOdd if even_odd else Fill.NonZero, Affine.IDENTITY, brush, None, self._path(contours))
        n, r = host_counts(contours)
        self.expect.append((n, r if records else None, int(even_odd)))
        self.k += 1
        self.words += 7 if gradient else 6
        return self

    def pairs(self, n, cols=3, rows=3):
        for _ in range(n):
            self.fill([rect_c(cols, rows, self.k, x=1 + self.k % 9, y=1 + (self.k // 9) % 9)])
        return self

    def solid(self, gradient=False):
        """A translucent cover of the whole target: SOLID + COLOR (3 words); gradient: SOLID + LIN_GRAD (4)."""
        from vello_amd import Affine, Fill, Gradient

        brush = colour(self.k, 40)
        if gradient:
            brush = Gradient.new_linear((0.0, 0.0), (12.0, 16.0)).with_stops([colour(self.k, 30), colour(self.k + 3, 70)])
            self.brushes = True
        self.s.fill(Fill.NonZero, Affine.IDENTITY, brush, None, self._cover())
        self.k += 1
        self.words += 4 if gradient else 3
        return self

    def push(self, contours=None):
        """BEGIN_CLIP (1 word) of a clip path that partially covers the tile (nearly all of it by default); its pop is FILL +
        END_CLIP (7 words).  (A clip that covers the tile altogether leaves no command in its list.)"""
        from vello_amd import Affine, Fill

        contours = contours or [rect_c(15, 15, len(self.open), x=0, y=0)]
        self.s.push_clip_layer(Fill.NonZero, Affine.IDENTITY, self._path(contours))
        self.open.append(contours)
        self.words += 1
        return self

    def pop(self):
        contours = self.open.pop()
        self.s.pop_layer()
        n, r = host_counts(contours)
        self.expect.append((n, r, 0))
        self.words += 7
        return self

    def filler(self, words):
        """`words` words of non-FILL commands: BEGIN_CLIPs (1 word each, closed at the list's end) and translucent SOLID + COLOR triples."""
        for _ in range(words % 3):
            self.push()
        for _ in range(words // 3):
            self.solid()
        return self

    def close(self):
        while self.open:
            self.pop()
        return self

    def resolve(self):
        """(packed, layout, resolved): resolved carries the ramps of a list with gradient brushes, None otherwise."""
        from vello_amd import Resolver

        self.close()
        if self.brushes:
            r = Resolver().resolve(self.s)
            return r.packed, r.layout, r
        return self.s.resolve() + (None,)


def render_and_plan(engine, tl, aa, name):
    """One frame of the list under `aa`; the engine's PTCL and segments; the expected FILLs checked against tile (0, 0)'s list."""
    packed, layout, resolved = tl.resolve()
    engine.set_auto_grow(True)
    img, bump = engine.render(packed, layout, tl.w, tl.h, BLACK, aa, ramps=resolved.ramps if resolved is not None else None)
    assert bump["failed"] == 0, f"{name}: {bump}"
    n_tiles = ((tl.w + 15) // 16) * ((tl.h + 15) // 16)
    ptcl = engine.read_buffer("ptcl", np.uint32, (64 * n_tiles + bump["ptcl"]) * 4)
    segments = engine.read_buffer("segments", np.uint32, bump["segments"] * 24).view(np.float32)
    c = engine.stage_constants()
    cmds, words = list_words(ptcl, 0, c)
    got = []
    for tag, at in cmds:
        if tag == CMD_FILL:
            n = int(ptcl[at + 1]) >> 1
            got.append((n, fill_records(segments, int(ptcl[at + 2]), n), int(ptcl[at + 1]) & 1))
    want = tl.expect
    assert len(got) == len(want), f"{name}: tile (0, 0) holds {len(got)} FILLs, the generator meant {len(want)}"
    for i, (g, w) in enumerate(zip(got, want)):
        assert all(b is None or a == b for a, b in zip(g, w)), f"{name}: FILL {i} is (segments, records, rule) {g}, meant {w}"
    n_words = sum(int(_CMD_SIZE[t]) for t, _ in cmds if t != CMD_JUMP)
    assert n_words == tl.words, f"{name}: the list holds {n_words} words, the generator meant {tl.words}"
    return packed, layout, resolved, ptcl, segments, c


def frames(engine, packed, layout, tl, aas, name, oracle, in_flight=1, order_sensitive=False, resolved=None):
    from vello_amd import AaConfig

    for aa in aas:
        compare_frame(engine, packed, layout, tl.w, tl.h, BLACK, aa, f"{name}_{int(aa)}_f{in_flight}", tol=1 if aa == AaConfig.Area else 0,
                      oracle=oracle, order_sensitive=order_sensitive and aa == AaConfig.Area, resolved=resolved)


def run_case(engine, tl, check, name, aas=None, in_flight=1, forced=False, order_sensitive=False, area_check=None):
    """The list rendered, `check(batches, fills, n_fills, c)` asserting the edge on the engine's own words, then every AA mode
    against the oracle."""
    from vello_amd import AaConfig

    aas = aas or (AaConfig.Msaa8, AaConfig.Msaa16)
    engine.set_frames_in_flight(in_flight)
    try:
        if forced:
            engine.set_debug_flags(fine_slices=True)
        first = [a for a in aas if a != AaConfig.Area] or [AaConfig.Area]
        packed, layout, resolved, ptcl, segments, c = render_and_plan(engine, tl, first[0], name)
        items = engine.fine_slice_stats()[0]
        if check is not None:
            check(plan_tile(ptcl, segments, 0, c), c, ptcl, segments, items)
        if area_check is not None:
            area_check(plan_area(ptcl, 0, c), c)
        frames(engine, packed, layout, tl, aas, name, make_oracle(), in_flight, order_sensitive or bool(layout.n_clips), resolved)
    finally:
        engine.set_frames_in_flight(1)
        if forced:
            engine.set_debug_flags()


def _paths(fills):
    return "".join({"simple": "s", "batch": "b", "unbatched": "u"}[f["path"]] for f in fills)


# ---------------------------------------------------------------------------------------------------------------
# (a) Fills a batch
# ---------------------------------------------------------------------------------------------------------------
REGULAR_COUNTS = (1, 2, 10, 11, 12, 23)


def check_regular(engine, n, name):
    """(FILL, COLOR) x n: a window shows the eleven FILLs at offsets 0, 6 .. 60 and the COLOR of the eleventh lies outside it."""
    def check(plan, c, *_):
        batches, fills, total = plan
        W = c["fine_window_words"]
        per = (W - 4) // 6 + 1
        assert total == n and len(fills) == n
        b = batches[0]
        assert b.s0 == 0 and b.shown == list(range(0, 6 * min(n, per), 6)) and b.kept == b.fit == min(n, per), f"{name}: {b}"
        assert b.fast == min(n, per if n > per else n, (W - 2 - 4) // 6 + 1), f"{name}: {b}"
        if n >= per:  # the eleventh FILL begins at the last offset a FILL may begin at; its COLOR begins outside the window
            assert b.shown[-1] == W - 4 and b.fast == per - 1 and fills[per - 1]["path"] == "batch", f"{name}: {b}"
        if n > per:  # the list resumes two words behind the window requested ahead
            b1 = batches[1]
            assert b1.how == "reused" and b1.base == b.base + W and b1.s0 == 2, f"{name}: {b1}"
        assert _paths(fills)[0] == "b" and (n < 2 or _paths(fills)[1] == "s")
        assert sum(b.fit or 1 for b in batches) == n

    run_case(engine, TileList().pairs(n), check, name)


NEST_DEPTHS = (11, 12, 13, 14)


def check_nested_clips(engine, depth, name):
    """`depth` nested clip layers whose clip paths partially cover the tile, a draw inside: BEGIN_CLIP x depth, FILL + COLOR, (FILL +
    END_CLIP) x depth -- FILLs seven words apart, the blend stack beyond its registers."""
    def check(plan, c, *_):
        batches, fills, total = plan
        assert total == depth + 1
        b = batches[0]
        assert b.how == "fresh" and b.shown == [0] + list(range(6, c["fine_window_words"] - 3, 7)), f"{name}: {b}"
        assert b.kept == len(b.shown) == 9 and b.fast == 1, f"{name}: {b}"
        assert all(len(x.shown) < c["fine_batch_fills"] for x in batches)

    tl = TileList()
    for i in range(depth):
        tl.push([rect_c(12 - i % 3, 13 - i % 4, i, x=1 + i % 2, y=1 + i % 3)])
    tl.pairs(1, 9, 9)
    run_case(engine, tl, check, name)


def check_densest_window(engine, name):
    """The densest list coarse writes shows fewer FILLs a window than fine_batch_fills: the fill limit is out of reach."""
    def check(plan, c, *_):
        batches, fills, total = plan
        assert max(len(b.shown) for b in batches) == (c["fine_window_words"] - 4) // 6 + 1 < c["fine_batch_fills"], batches

    run_case(engine, TileList().pairs(40, 2, 2), check, name)


MIXED_CASES = {"end_clip_0": ("end_clip", 0), "solid_1": ("solid", 1), "solid_n-1": ("solid", 9), "clip_1": ("clip", 1), "clip_n-1": ("clip", 9),
               "gradient_0": ("gradient", 0), "gradient_1": ("gradient", 1), "gradient_n-1": ("gradient", 9)}


def check_mixed(engine, case, name):
    """Ten fills in a window of which the regular prefix holds 0, 1 or 9: behind it a SOLID + COLOR or a BEGIN_CLIP stands between two
    pairs, or the next fill's draw command is a gradient or an END_CLIP."""
    kind, at = MIXED_CASES[case]
    tl = TileList().pairs(at)
    if kind == "gradient":
        tl.fill([rect_c(5, 6, 3)], gradient=True)
    elif kind == "end_clip":
        tl.push([rect_c(7, 6, 3)]).pop()
    else:
        tl.solid() if kind == "solid" else tl.push()
        tl.pairs(1)
    tl.pairs(9 - at)

    def check(plan, c, *_):
        batches, fills, total = plan
        b = batches[0]
        assert b.s0 == 0 and b.fast == at and b.fit == len(b.shown) >= 10, f"{name}: {b}"
        assert fills[at]["path"] == "batch" and fills[at]["batch"] == 0, f"{name}: {fills[at]}"

    run_case(engine, tl, check, name)


# ---------------------------------------------------------------------------------------------------------------
# (b) Segments a batch
# ---------------------------------------------------------------------------------------------------------------
SEGMENT_SPLITS = {"last": lambda t: [20, 20, t - 40], "middle": lambda t: [30, t - 30, 4, 4], "second": lambda t: [t - 5, 5, 4]}


def check_segment_sum(engine, where, delta, name):
    """Fills whose segments sum to fine_batch_segments + delta at the fill the case names; the fills behind it are small."""
    c = engine.stage_constants()
    lim = c["fine_batch_segments"]
    counts = SEGMENT_SPLITS[where](lim + delta)
    edge = {"last": 2, "middle": 1, "second": 1}[where]
    tl = TileList()
    for i, n in enumerate(counts):
        tl.fill([ngon_c(n, i, 5.5 - 0.4 * i)], records=False)

    def check(plan, c, *_):
        batches, fills, total = plan
        b = batches[0]
        assert b.segs == counts and sum(counts[: edge + 1]) == lim + delta, f"{name}: {b}"
        assert b.kept == (len(counts) if delta <= 0 and sum(counts) <= lim else edge if delta > 0 else b.kept), f"{name}: {b}"
        if delta > 0:
            assert b.kept == edge and batches[1].s0 in (0, 2) and batches[1].segs[0] == counts[edge], f"{name}: {batches}"
        else:
            assert b.kept > edge, f"{name}: {b}"

    run_case(engine, tl, check, name)


SINGLE_SEGMENTS = (63, 64, 65, 128, 129)


def check_single_fill_segments(engine, n, second, name):
    """One fill of n segments as the first fill of its batch (second: behind a small fill, so that the batch ends in front of it):
    up to fine_batch_segments it is staged alone, beyond it goes unbatched in rounds of 64."""
    tl = TileList()
    if second:
        tl.pairs(1)
    tl.fill([ngon_c(n, 1)], records=False)
    tl.pairs(2)

    def check(plan, c, *_):
        batches, fills, total = plan
        lim = c["fine_batch_segments"]
        i = 1 if second else 0
        f = fills[i]
        b = batches[f["batch"]]
        assert f["segs"] == n and f["off"] == b.s0, f"{name}: fill {i} is not the first of its batch: {f} {b}"
        if second:
            assert batches[0].kept == 1 and batches[0].segs[1] == n, f"{name}: {batches[0]}"
        if n <= lim:
            assert b.kept >= 1 and f["path"] in ("batch", "simple") and (n + 4 <= lim or b.kept == 1), f"{name}: {b}"
        else:
            assert b.kept == 0 and b.prefetch is None and f["path"] == "unbatched" and fills[i + 1]["path"] == "batch", f"{name}: {b}"

    run_case(engine, tl, check, name)


# ---------------------------------------------------------------------------------------------------------------
# (c) Records a batch
# ---------------------------------------------------------------------------------------------------------------
def check_record_cap(engine, where, delta, name):
    """The kept fills' records end at fine_item_cap + delta: inside the last fill of the window, inside a middle one, or with the
    first fill alone (its successor fits)."""
    c = engine.stage_constants()
    cap = c["fine_item_cap"] + delta
    tl = TileList()
    if where == "first":
        tl.fill(tuned_c(cap, 26))
        tl.pairs(3)
        edge = 0
    else:
        each = host_counts([tall_c(5)])[1]
        for i in range(4):
            tl.fill([tall_c(5, i)])
        tl.fill(tuned_c(cap - 4 * each, 3, 5))
        edge = 4
        if where == "middle":
            tl.pairs(3)

    def check(plan, c, *_):
        batches, fills, total = plan
        b = batches[0]
        assert b.kept == len(b.shown) == total and b.ends[edge] == cap, f"{name}: {b}"
        if delta <= 0 and where == "last":
            assert b.fit == total, f"{name}: {b}"
        if delta <= 0 and where != "last":  # the fills behind it are over the cap
            assert b.fit == edge + 1 and b.ends[edge + 1] > c["fine_item_cap"], f"{name}: {b}"
        if delta > 0:
            assert b.fit == edge
            if edge == 0:  # the first fill alone is over the cap: unbatched, and the window requested ahead is of no use
                assert fills[0]["path"] == "unbatched" and batches[1].how == "fresh" and batches[1].fit == 3, f"{name}: {batches}"
            else:
                assert batches[1].how == "fresh" and batches[1].s0 == 0 and fills[edge]["batch"] == 1, f"{name}: {batches}"
        if delta <= 0 and where == "first":  # the next batch begins in front of the window requested ahead: a fresh one
            assert fills[0]["path"] == "batch" and batches[1].how == "fresh" and batches[1].base < b.prefetch, f"{name}: {batches}"

    run_case(engine, tl, check, name)


# ---------------------------------------------------------------------------------------------------------------
# (d) The simple-fill edge
# ---------------------------------------------------------------------------------------------------------------
SIMPLE_RECORDS = (1, 2, 63, 64, 65)


def _few_records_fill(tl, records):
    """A fill of 1 or 2 records: a triangle with two corners in the tile to the right and one side on an integer row (of that side
    a segment without a crossing, of the diagonal a piece inside one pixel of this tile), a sliver inside one pixel.  (No list
    holds a FILL without a record: path_count drops a path's horizontal lines, and any other segment crosses a pixel.)"""
    if records == 1:
        tl.fill([[(15.5, 3.0), (16.5, 3.0), (16.5, 3.5)]], records=False)
        tl.expect[-1] = (2, 1, 0)
    else:
        tl.fill([[(2.2, 3.0), (2.8, 3.0), (2.5, 3.6)]])


def check_simple_records(engine, records, name):
    """A non-zero fill of `records` records as the third fill of a regular prefix: 1 .. fine_simple_records takes the straight-line
    replay, more the general one."""
    tl = TileList(32 if records == 1 else 16, 16)
    tl.pairs(2)
    if records <= 2:
        _few_records_fill(tl, records)
    else:
        tl.fill(exact_c(records, 3))
    tl.pairs(2)

    def check(plan, c, *_):
        batches, fills, total = plan
        f = fills[2]
        assert batches[0].fast == 5 and f["records"] == records, f"{name}: {f} {batches[0]}"
        assert f["path"] == ("simple" if 1 <= records <= c["fine_simple_records"] else "batch"), f"{name}: {f}"
        assert _paths(fills) == "bs" + ("s" if f["path"] == "simple" else "b") + "ss", _paths(fills)

    run_case(engine, tl, check, name)


def check_simple_handoff(engine, kind, name):
    """An even-odd fill or a fill of more than fine_simple_records records between two runs of simple fills: the run ends, the
    general replay clears or keeps the counters, the next run starts with its records requested ahead."""
    tl = TileList()
    tl.pairs(3)
    if kind == "even_odd":
        tl.fill([rect_c(9, 8, 2), rect_c(4, 4, 3, 3, 3)], even_odd=True)
    else:
        tl.fill(exact_c(engine.stage_constants()["fine_simple_records"] + 31, 3))
    tl.pairs(3)

    def check(plan, c, *_):
        batches, fills, total = plan
        assert batches[0].fast == 7 and batches[0].fit == 7, batches[0]
        # after an even-odd fill the counters are dirty: the fill behind it takes the general replay once more
        assert _paths(fills) == ("bssbbss" if kind == "even_odd" else "bssbsss"), _paths(fills)

    run_case(engine, tl, check, name)


# ---------------------------------------------------------------------------------------------------------------
# (e) Windows
# ---------------------------------------------------------------------------------------------------------------
WINDOW_OFFSETS = (57, 58, 59, 60, 61)


def check_window_offset(engine, off, name):
    """Eleven pairs (the window's eleven FILLs; the interpreter loads its next window at the COLOR behind the last, which is where
    the window requested ahead begins), off - 56 words of non-FILL commands, twelve pairs: the second batch takes the window
    requested ahead, its regular prefix begins at off - 54 and its tenth FILL at window offset `off`, the COLOR behind it at
    off + 4."""
    s0 = off - 54
    tl = TileList().pairs(11).filler(s0 - 2).pairs(12)

    def check(plan, c, *_):
        batches, fills, total = plan
        W = c["fine_window_words"]
        b0, b1 = batches[0], batches[1]
        assert b0.kept == 11 and b0.fast == 10 and b1.how == "reused" and b1.base == b0.base + W and b1.s0 == s0, f"{name}: {batches[:2]}"
        if off <= W - 4:
            assert b1.shown[-1] == off and b1.kept == 10, f"{name}: {b1}"
            assert b1.fast == (10 if off + 4 <= W - 2 else 9), f"{name}: {b1}"  # the COLOR at 61, 62 is inside, at 63, 64 outside
            assert fills[20]["off"] == off and fills[20]["path"] == ("simple" if b1.fast == 10 else "batch")
        else:
            assert b1.shown[-1] == off - 6 and b1.kept == 9 and b1.fast == 9, f"{name}: {b1}"
            assert fills[20]["batch"] == 2 and fills[20]["off"] == batches[2].s0, f"{name}: the FILL at offset {off} did not start a window: {batches[2]}"

    run_case(engine, tl, check, name)


REACH_DELTAS = (-1, 0, 1, "far")


def check_prefetch_reach(engine, delta, name):
    """Two batches fine_prefetch_reach + delta words apart: up to the reach the window requested ahead is taken, beyond it a fresh
    one is loaded.  far: one pair, then fine_window_words - 2 words to the next FILL, whose own words would lie outside the window
    requested ahead (the interpreter has loaded a window of its own at a SOLID by then, so the planner does have to choose)."""
    c = engine.stage_constants()
    far = delta == "far"
    gap = c["fine_window_words"] - 2 if far else c["fine_prefetch_reach"] + delta
    first = 1 if far else 11
    tl = TileList().pairs(first).filler(gap - 2).pairs(6)

    def check(plan, c, *_):
        batches, fills, total = plan
        b1 = batches[1]
        assert batches[0].kept == first and batches[0].prefetch == batches[0].base + 6 * first - 2, f"{name}: {batches[0]}"
        if gap <= c["fine_prefetch_reach"]:
            assert b1.how == "reused" and b1.s0 == gap, f"{name}: {b1}"
        else:  # ("fresh": the planner looked at the window requested ahead and refused it)
            assert b1.how == "fresh" and b1.s0 == 0 and b1.base == batches[0].prefetch + gap, f"{name}: {b1}"
        assert fills[first]["batch"] == 1 and total == first + 6 + (gap - 2) % 3

    run_case(engine, tl, check, name)


JUMP_CASES = {"first_block_full": 10, "first_block_9": 9, "jump_before_fill": 0}


def check_jump(engine, case, name):
    """The tile's fixed block: a list of exactly the block's room stays in it (the last FILL's COLOR ends at the two headroom words);
    a longer one is a region of its own behind a CMD_JUMP in the block's first command word -- a JUMP directly in front of a FILL."""
    n = {"first_block_full": 10, "first_block_9": 9, "jump_before_fill": 11}[case]
    tl = TileList().pairs(n)

    def check(plan, c, ptcl, *_):
        batches, fills, total = plan
        cmds, words = list_words(ptcl, 0, c)
        assert words == 6 * n
        if n <= 10:
            assert all(t != CMD_JUMP for t, _ in cmds) and cmds[-1][1] == 1 + 6 * n and batches[0].base == 1, f"{name}: {cmds[-1]} {batches[0]}"
            assert 1 + 6 * n + 1 <= c["ptcl_initial_alloc"] - 2 + 1
        else:
            assert cmds[0][0] == CMD_JUMP and cmds[1][0] == CMD_FILL and batches[0].how == "same" and batches[0].base == cmds[1][1], f"{name}: {batches[0]}"

    run_case(engine, tl, check, name)


def check_jump_behind_batch(engine, first, name):
    """More draws than a batch of coarse's: `first` pairs of the first batch stay in the tile's fixed block, the pairs of the second
    batch do not fit behind them -- a CMD_JUMP directly behind a pair's COLOR, a continuation region that begins with a FILL."""
    from vello_amd import Affine, Fill, Rect

    c = engine.stage_constants()
    tl = TileList(32, 16).pairs(first)
    for i in range(c["coarse_batch"] - first):  # the rest of coarse's batch lies in the tile to the right
        tl.s.fill(Fill.NonZero, Affine.IDENTITY, colour(i, 30), None, Rect(17.2 + (i % 11), 1.2 + (i // 11) % 12, 19.1 + (i % 11), 3.3 + (i // 11) % 12))
    tl.pairs(12)

    def check(plan, c, ptcl, *_):
        batches, fills, total = plan
        cmds, words = list_words(ptcl, 0, c)
        tags = [t for t, _ in cmds]
        j = tags.index(CMD_JUMP)
        assert tags.count(CMD_JUMP) == 1 and j == 2 * first and cmds[j][1] == 1 + 6 * first and tags[j + 1] == CMD_FILL, f"{name}: {cmds[:2 * first + 3]}"
        assert batches[0].shown == list(range(0, 6 * first, 6)) and batches[0].fast == first, f"{name}: {batches[0]}"
        assert batches[1].how == "same" and batches[1].base == cmds[j + 1][1] and len(batches[1].shown) == 11, f"{name}: {batches[1]}"

    run_case(engine, tl, check, name)


# ---------------------------------------------------------------------------------------------------------------
# (f) Slices
# ---------------------------------------------------------------------------------------------------------------
def slice_items(n_fills, slice_fills, min_fills):
    return (n_fills + slice_fills - 1) // slice_fills if n_fills >= min_fills else 0


def _check_slices(name, n, key_fills, key_min, prefix_cut=None):
    def check(plan, c, ptcl, segments, items):
        batches, fills, total = plan
        sf, mn = c[key_fills], c[key_min]
        want = slice_items(total, sf, mn)
        assert total == n and items == want, f"{name}: {items} slice items for {total} fills, not {want}"
        taken = []
        for k in range(want):  # every slice's own walk: its fills, all of them, once
            b, f, _ = plan_tile(ptcl, segments, 0, c, k * sf, (k + 1) * sf if k + 1 < want else None)
            assert [x["no"] for x in f] == list(range(k * sf, min((k + 1) * sf, total))), f"{name}: slice {k} takes {[x['no'] for x in f]}"
            taken.append((b, f))
        if prefix_cut is not None:
            prefix_cut(taken, c)

    return check


FORCED_FILLS = (4, 5, 8, 9, 12, 13)


def check_slices_forced(engine, n, in_flight, name):
    """n fills under fine_slices=True: slices of 4 from 5 fills on, on a target of four tiles (as many slice items as fit at most)."""
    tl = TileList(32, 32).pairs(n)
    run_case(engine, tl, _check_slices(name, n, "fine_slice_fills_forced", "fine_slice_min_fills_forced"), name, in_flight=in_flight, forced=True)


def check_slices_natural(engine, delta, in_flight, name):
    """fine_slice_min_fills + delta small fills in one tile (the in-flight threshold with two frames in flight)."""
    c = engine.stage_constants()
    key = "fine_slice_min_fills" if in_flight == 1 else "fine_slice_min_fills_in_flight"
    n = c[key] + delta
    tl = TileList(64 if in_flight == 2 else 32, 32).pairs(n, 2, 2)  # (slice items never outnumber the target's tiles: eight for seven items)
    run_case(engine, tl, _check_slices(name, n, "fine_slice_fills", key), name, in_flight=in_flight)


SLICE_END_CASES = ("inside_prefix", "prefix_end", "batch_end", "behind_clips", "last_of_one")


def check_slice_end(engine, case, name):
    """Forced slices of four fills whose first slice ends inside a batch's regular prefix, at the prefix's end, at the batch's end;
    a slice whose first fill stands behind clip commands, the clip opened in an earlier slice and closed in a later one; a last
    slice of one fill."""
    tl = TileList(32, 32)
    if case == "inside_prefix":
        tl.pairs(9)
    elif case == "prefix_end":
        tl.pairs(4).solid().pairs(4)
    elif case == "batch_end":
        tl.pairs(3).fill([ngon_c(50, 1)], records=False).fill([ngon_c(40, 2)], records=False).pairs(3)
    elif case == "behind_clips":
        tl.pairs(3).push([rect_c(11, 12, 1)]).pairs(1).push([rect_c(9, 9, 2)]).solid().pairs(5).pop().pop().pairs(2)
    else:
        tl.pairs(9)

    def cut(taken, c):
        b0 = taken[0][0][0]
        if case == "inside_prefix":
            assert b0.fast == 9 and b0.cut == 5, b0
        elif case == "prefix_end":
            assert b0.fast == 4 and b0.cut == 0 and len(b0.shown) > 4, b0
        elif case == "batch_end":
            assert b0.kept == 4 and b0.fit == 4 and len(b0.shown) > 4, b0
        elif case == "behind_clips":
            b1 = taken[1][0][0]
            assert b1.how == "fresh" and taken[1][1][0]["no"] == 4, b1
        else:
            assert len(taken) == 3 and len(taken[2][1]) == 1, taken[2]

    n = len(tl.close().expect)
    run_case(engine, tl, _check_slices(name, n, "fine_slice_fills_forced", "fine_slice_min_fills_forced", cut), name, forced=True)


def check_slices_mixed_tiles(engine, in_flight, name):
    """Two sliced tiles and one unsliced tile in one frame of four tiles: nine fills in tile (0, 0), six in (1, 1), three in (1, 0)."""
    from vello_amd import Affine, Fill, Rect

    tl = TileList(32, 32).pairs(9)
    for i in range(9):
        if i < 6:
            tl.s.fill(Fill.NonZero, Affine.IDENTITY, colour(20 + i), None, Rect(17.3 + i, 17.2 + i, 22.4 + i, 23.9 + 0.5 * i))
        if i < 3:
            tl.s.fill(Fill.EvenOdd, Affine.IDENTITY, colour(40 + i), None, Rect(18.3 + i, 2.2 + i, 25.4 + i, 9.9 + 0.5 * i))

    def check(plan, c, ptcl, segments, items):
        counts = [plan_tile(ptcl, segments, t, c)[2] for t in range(4)]
        assert counts == [9, 3, 0, 6] and items == 3 + 2, f"{name}: fills per tile {counts}, {items} slice items"

    run_case(engine, tl, check, name, in_flight=in_flight, forced=True)


# ---------------------------------------------------------------------------------------------------------------
# (g) Dispatch order
# ---------------------------------------------------------------------------------------------------------------
def dispatch_lengths(c):
    b, n = c["fine_bucket_words"], c["fine_buckets"]
    return [b + d for d in (-1, 0, 1)] + [b * (n - 1) + d for d in (-1, 0, 1)] + [c["fine_heavy_words"] + d for d in (-1, 0, 1)]


def check_dispatch(engine, which, name):
    """Four tiles whose lists are L - 1, L, L + 1 and 6 words long, L a bucket's edge or the heavy threshold: every tile rendered
    exactly once, into a target cleared to a value no pixel of the frame takes."""
    from vello_amd import AaConfig, Affine, Fill, Gradient, Rect, Resolver, Scene

    c = engine.stage_constants()
    L = {"bucket_1": c["fine_bucket_words"], "last_bucket": c["fine_bucket_words"] * (c["fine_buckets"] - 1), "heavy": c["fine_heavy_words"]}[which]
    s = Scene()
    want = []
    k = 0
    for t, words in enumerate((L - 1, L, L + 1, 6)):
        ox, oy = 16.0 * (t % 2), 16.0 * (t // 2)
        grads = words % 2  # words = 7 gradient fills (FILL + LIN_GRAD) + 8 clip layers (BEGIN_CLIP, FILL + END_CLIP) + 6 pairs
        clips = (2 * ((words - 7 * grads) % 3)) % 3
        pairs, rest = divmod(words - 7 * grads - 8 * clips, 6)
        assert pairs >= 0 and rest == 0
        for i in range(grads):
            g = Gradient.new_linear((ox, oy), (ox + 16.0, oy + 12.0)).with_stops([colour(k, 90), colour(k + 5, 200)])
            s.fill(Fill.NonZero, Affine.IDENTITY, g, None, Rect(ox + 2.3, oy + 3.2, ox + 12.6, oy + 11.7))
            k += 1
        for i in range(clips):
            s.push_clip_layer(Fill.NonZero, Affine.IDENTITY, Rect(ox + 0.4 + i, oy + 0.6, ox + 15.2, oy + 15.5 - i))
        for i in range(pairs):
            s.fill(Fill.NonZero, Affine.IDENTITY, colour(k), None, Rect(ox + 1.3 + i % 9, oy + 1.2 + (i // 9) % 9, ox + 4.6 + i % 9, oy + 5.1 + (i // 9) % 9))
            k += 1
        for i in range(clips):
            s.pop_layer()
        want.append(words)
    resolved = Resolver().resolve(s)
    packed, layout = resolved.packed, resolved.layout
    engine.set_auto_grow(True)
    sentinel = 0xFF0BADF0  # an empty frame of this colour first: a tile fine leaves out keeps it
    blank = Scene().resolve()
    engine.render(blank[0], blank[1], 32, 32, sentinel, AaConfig.Msaa8)
    img, bump = engine.render(packed, layout, 32, 32, BLACK, AaConfig.Msaa8, ramps=resolved.ramps)
    assert bump["failed"] == 0
    assert not (img.view(np.uint32)[:, :, 0] == sentinel).any(), f"{name}: a tile was not rendered"
    ptcl = engine.read_buffer("ptcl", np.uint32, (64 * 4 + bump["ptcl"]) * 4)
    got = [list_words(ptcl, t, c)[1] for t in range(4)]
    assert got == want, f"{name}: list lengths {got}, meant {want}"
    ctl = engine.control_words()[16:48]
    buckets = [min(c["fine_buckets"] - 1, w // c["fine_bucket_words"]) for w in want]
    assert [int(ctl[b]) for b in sorted(set(buckets))] == [buckets.count(b) for b in sorted(set(buckets))] and int(ctl.sum()) == 4, f"{name}: {ctl}"
    o = make_oracle()
    for aa in (AaConfig.Msaa8, AaConfig.Msaa16, AaConfig.Area):
        engine.render(blank[0], blank[1], 32, 32, sentinel, aa)
        frames(engine, packed, layout, TileList(32, 32), (aa,), name, o, order_sensitive=True, resolved=resolved)


# ---------------------------------------------------------------------------------------------------------------
# (h) Winding at the byte's edge
# ---------------------------------------------------------------------------------------------------------------
WINDINGS = (126, 127, 128, 129)


WINDING_KINDS = ("crossings_unbatched", "rows_unbatched", "backdrop_unbatched", "backdrop_staged")


def _wound(turns, kind):
    """`turns` nested rectangles of one direction.  crossings: all inside the tile, the x winding prefix itself passes the byte's
    edge (four segments a turn).  rows: their left edges lie left of the target, their upper and lower edges cross the tile's left
    edge -- the row counters pass the byte's edge (three segments a turn, backdrop 0).  backdrop: their upper edges lie above the
    target as well, the FILL's backdrop is `turns` (two segments a turn); staged: all but the innermost cover the target altogether and the innermost's right edge alone crosses the tile -- one
    segment, so that the fill is staged and its row counters and zero_at are formed with a backdrop beyond the byte."""
    out = []
    for i in range(turns):
        d = 0.04 * i
        if kind == "crossings_unbatched":
            out.append([(2.2 + d, 2.3 + d / 2), (13.7 - d, 2.3 + d / 2), (13.7 - d, 13.6 - d / 2), (2.2 + d, 13.6 - d / 2)])
        elif kind == "backdrop_unbatched":
            out.append([(-6.0 + d, -4.0 - d), (13.7 - d, -4.0 - d), (13.7 - d, 13.6 - d / 2), (-6.0 + d, 13.6 - d / 2)])
        elif kind == "rows_unbatched":
            out.append([(-6.0 + d, 2.3 + d / 2), (13.7 - d, 2.3 + d / 2), (13.7 - d, 13.6 - d / 2), (-6.0 + d, 13.6 - d / 2)])
        else:
            x1 = 9.7 if i == turns - 1 else 24.0 + d
            out.append([(-6.0 + d, -4.0 - d), (x1, -4.0 - d), (x1, 21.0 + d), (-6.0 + d, 21.0 + d)])
    return out


def check_winding(engine, turns, kind, reverse, name):
    """A non-zero path that winds `turns` times round pixels of the tile (reverse: the other way round), between two small fills."""
    contours = _wound(turns, kind)
    if reverse:
        contours = [p[::-1] for p in contours]
    tl = TileList().pairs(1).fill(contours, records=False)
    n_segs = {"crossings_unbatched": 4 * turns, "rows_unbatched": 3 * turns, "backdrop_unbatched": 2 * turns, "backdrop_staged": 1}[kind]
    tl.expect[-1] = (n_segs, None, 0)
    tl.pairs(1)

    def check(plan, c, ptcl, *_):
        batches, fills, total = plan
        f = fills[1]
        bd = int(np.int32(ptcl[f["at"] + 3]))
        # (vello's rectangles run clockwise in y-down coordinates; the sign follows the direction)
        assert abs(bd) == (turns if kind.startswith("backdrop") else 0), f"{name}: backdrop {bd}"
        assert (f["path"] != "unbatched") == (kind == "backdrop_staged") and f["batch"] == (0 if kind == "backdrop_staged" else 1), f"{name}: {f}"
        return bd

    run_case(engine, tl, check, name)


# ---------------------------------------------------------------------------------------------------------------
# (i) Area AA
# ---------------------------------------------------------------------------------------------------------------
AREA_SEGMENTS = (63, 64, 65, 129)


def check_area_segments(engine, n, name):
    """A fill of n segments between small fills: rounds of 64; requested ahead by its predecessor up to 64 segments of it."""
    from vello_amd import AaConfig

    tl = TileList().pairs(1).fill([ngon_c(n, 1)], records=False).pairs(1)

    def area(fills, c):
        assert [f["segs"] for f in fills] == [4, n, 4] and fills[0]["ahead"][1] == n and fills[1]["ahead"][1] == 4, fills

    run_case(engine, tl, None, name, aas=(AaConfig.Area,), area_check=area)


AREA_LOOKAHEAD = (58, 59, 60, 61)


def check_area_lookahead(engine, off, name):
    """A next FILL that begins at window offset `off` behind a COLOR: requested ahead while its four words lie inside the window."""
    from vello_amd import AaConfig

    r = off % 6
    tl = TileList().filler(r).pairs(14)

    def area(fills, c):
        W = c["fine_window_words"]
        hit = [f for f in fills if f["next_fill_off"] == off]
        assert hit, f"{name}: no next FILL at offset {off}: {[f['next_fill_off'] for f in fills]}"
        assert all((f["ahead"] is not None) == (off + 4 <= W) for f in hit), f"{name}: {hit}"

    run_case(engine, tl, None, name, aas=(AaConfig.Area,), area_check=area, order_sensitive=True)
