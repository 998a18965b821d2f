"""The Update family (rtx_update, rtx_update_begin / _end, rtx_update_delta, rtx_update_half) as one table: every delivery form
hands over the oracle's minimised bytes and moves the statistics by what the form implies; every refusal has its code, its message,
its physics step or none, and its effect on the next delta frame; and a mixed sequence of the entry points equals the oracle frame
by frame.  What the entry points do differently from one another ("Known divergences") is pinned here as it is."""
import ctypes as C

import numpy as np
import pytest

import oracle as O
import restate_delta as RD
import restate_half as RH
import util as U

pytestmark = pytest.mark.gpu

CW, CH = 64, 48                     # the context
SIZES = [(37, 21), (64, 48)]        # one Minimize block, three
DT = 0.05


@pytest.fixture(scope="module")
def R():
    return U.pkg()


@pytest.fixture(scope="module")
def ctx(R):
    c = R.Context(CW, CH)
    c.set_reference_default_scene()
    yield c
    c.close()


@pytest.fixture(scope="module")
def pinned(ctx):
    # three destinations, each large enough for any stream of a CW x CH console (a half-block frame's bound: 41 bytes per cell)
    bufs = [ctx.host_alloc(41 * CW * CH + 16) for _ in range(3)]
    yield bufs
    for ptr, _ in bufs:
        ctx.host_free(ptr)


_want = {}


def want_stream(R, size, mode):
    """The oracle's Update of the default scene at rest, computed once per (size, mode)."""
    if (size, mode) not in _want:
        p = R.camera_params(*size)
        _want[(size, mode)] = O.minimize(mode, O.render(U.oracle_params(p), O.Scene.reference_default(), mode), *size)
    return _want[(size, mode)]


# name, options, pipelined, destination, host writes per frame of a character mode
FORMS = [
    ("blocking copy", {"OPT_UPDATE_HOST_WRITE": 0}, False, "pinned", 0),
    ("blocking host-write", {}, False, "pinned", 1),
    ("blocking host-write asked for", {"OPT_UPDATE_HOST_WRITE": 1}, False, "pinned", 1),
    ("blocking, destination not 16-byte aligned", {}, False, "unaligned", 0),
    ("blocking, pageable destination", {}, False, "pageable", 0),
    ("blocking records", {"OPT_UPDATE_WORDS": 0}, False, "pinned", 0),
    ("blocking, three launches", {"OPT_MINIMIZE_FUSED": 0}, False, "pinned", 0),
    ("blocking, blocks give up", {"OPT_MINIMIZE_FUSED": 2}, False, "pinned", 1),
    ("pipelined copy", {"OPT_UPDATE_HOST_WRITE": 0}, True, "pinned", 0),
    ("pipelined host-write", {}, True, "pinned", 1),
    ("pipelined, destination not 16-byte aligned", {}, True, "unaligned", 0),
    ("pipelined records", {"OPT_UPDATE_WORDS": 0}, True, "pinned", 0),
    ("pipelined, three launches", {"OPT_MINIMIZE_FUSED": 0}, True, "pinned", 0),
    ("pipelined, blocks give up", {"OPT_MINIMIZE_FUSED": 2}, True, "pinned", 1),
]


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("mode", range(6))
def test_every_delivery_form_hands_over_the_oracles_stream(R, ctx, pinned, mode, size):
    W, H = size
    p = R.camera_params(W, H)
    want = want_stream(R, size, mode)
    assert want.size > 0
    pageable = [np.zeros(20 * CW * CH, dtype=np.uint8) for _ in range(2)]
    for name, options, pipelined, where, writes in FORMS:
        what = (name, R.MODE_NAMES[mode], size)
        dst = []
        for k in range(2):
            if where == "pageable":
                dst.append((pageable[k].ctypes.data, pageable[k]))
            else:
                off = 4 if where == "unaligned" else 0
                dst.append((pinned[k][0] + off, pinned[k][1][off:]))
            dst[k][1][:want.size + 8] = 0xEE
        for opt, v in options.items():
            ctx.set_option(getattr(R, opt), v)
        try:
            w0, f0 = ctx.get_option(R.STAT_UPDATE_HOST_WRITES), ctx.get_option(R.STAT_MINIMIZE_FALLBACKS)
            n = C.c_size_t()
            if pipelined:
                frames = 2  # both slots in flight
                t0 = ctx.update_begin(p, mode, dst[0][0])
                t1 = ctx.update_begin(p, mode, dst[1][0])
                assert {t0, t1} == {0, 1}, what
                got = [dst[k][1][:ctx.update_end(t)].copy() for k, t in enumerate((t0, t1))]
            else:
                frames = 1
                ctx._check(R.lib().rtx_update(ctx._h, C.byref(p), mode, 0.0, 0, C.c_void_p(dst[0][0]), C.byref(n)))
                got = [dst[0][1][:n.value].copy()]
            for k, g in enumerate(got):
                assert g.size == want.size and np.array_equal(g, want), what
                assert (dst[k][1][want.size:want.size + 8] == 0xEE).all(), what
            # SDL has no pixel words: the record form, which never writes the host itself
            assert ctx.get_option(R.STAT_UPDATE_HOST_WRITES) - w0 == (0 if mode == R.SDL else writes * frames), what
            # (rtx_min_fused under option 2: every block b with b % 3 == 1 gives up, so a frame of two blocks or more is redone)
            gave_up = options.get("OPT_MINIMIZE_FUSED") == 2 and W * H > 1024
            assert ctx.get_option(R.STAT_MINIMIZE_FALLBACKS) - f0 == (frames if gave_up else 0), what
        finally:
            for opt in options:
                ctx.set_option(getattr(R, opt), -1)


# ---- refusals

def copy_params(R, p, x=None, y=None):
    q = R.Params.from_buffer_copy(bytes(p))
    if x is not None:
        q.x = x
    if y is not None:
        q.y = y
    return q


class Caller:
    """The five entry points called as the C ABI has them, on a context whose oracle twin steps with it."""

    def __init__(self, R, c, host):
        self.R, self.c, self.host, self.sc = R, c, host, O.Scene.reference_default()
        self.n, self.ticket, self.kind = C.c_size_t(), C.c_int(-1), C.c_int(-1)

    def call(self, entry, p, mode, physics=True, capacity=1 << 30, dst=0):
        L, h = self.R.lib(), self.c._h
        ptr = C.c_void_p(self.host[dst][0])
        if entry == "update":
            rc = L.rtx_update(h, C.byref(p), mode, DT, int(physics), ptr, C.byref(self.n))
        elif entry == "begin":
            rc = L.rtx_update_begin(h, C.byref(p), mode, DT, int(physics), ptr, C.byref(self.ticket))
        elif entry == "delta":
            rc = L.rtx_update_delta(h, C.byref(p), mode, DT, int(physics), 0, ptr, capacity, C.byref(self.n), C.byref(self.kind))
        else:
            assert entry == "half"
            rc = L.rtx_update_half(h, C.byref(p), mode, DT, int(physics), ptr, capacity, C.byref(self.n))
        return rc, (L.rtx_last_error(h) or b"").decode()

    def end(self, ticket):
        L, h = self.R.lib(), self.c._h
        rc = L.rtx_update_end(h, ticket, C.byref(self.n))
        return rc, (L.rtx_last_error(h) or b"").decode()

    def step_oracle(self):
        O.lib().orc_update_objects(self.sc.ptrs(), self.sc.count, DT)

    def physics_agrees(self):
        """Sphere 0 is where the oracle's stepped scene has it: one step more or less shows."""
        return self.c.get_object(0)[1][1] == np.float32(self.sc.objects()[0].center.y)

    def next_delta_kind(self, p, mode):
        rc, msg = self.call("delta", p, mode, physics=False, dst=2)  # (a destination no frame in flight is written to)
        assert rc == 0, msg
        return self.kind.value


TOO_LARGE_MSG = "frame larger than the context was created for"
DELTA_RANGE_MSG = "rtx_update_delta: x - 1 and y must be in [0, 99999], x and y at least 1"
HALF_RANGE_MSG = "rtx_update_half: x and 2 y must be in [1, 2^31)"
HALF_LARGE_MSG = "rtx_update_half: W x 2H pixels are more than the context was created for (create it with twice the rows)"

# entry, case, status, message, the physics step ran, the next delta is a key frame
REFUSALS = [
    ("update", "mode -1", "ERR_INVALID_MODE", "invalid rendering mode", True, True),
    ("update", "mode 6", "ERR_INVALID_MODE", "invalid rendering mode", True, True),
    ("update", "x = 0", "ERR_INVALID_ARGUMENT", TOO_LARGE_MSG + ", or empty", True, True),
    ("update", "over capacity", "ERR_TOO_LARGE", TOO_LARGE_MSG + ", or empty", True, True),
    ("begin", "mode -1", "ERR_INVALID_MODE", "invalid rendering mode", False, True),
    ("begin", "mode 6", "ERR_INVALID_MODE", "invalid rendering mode", False, True),
    ("begin", "x = 0", "ERR_TOO_LARGE", TOO_LARGE_MSG, False, True),
    ("begin", "over capacity", "ERR_TOO_LARGE", TOO_LARGE_MSG, False, True),
    ("delta", "mode -1", "ERR_INVALID_MODE", "rtx_update_delta: not a character mode", False, False),
    ("delta", "mode 6", "ERR_INVALID_MODE", "rtx_update_delta: not a character mode", False, False),
    ("delta", "SDL", "ERR_INVALID_MODE", "rtx_update_delta: not a character mode", False, False),
    ("delta", "x = 0", "ERR_INVALID_ARGUMENT", DELTA_RANGE_MSG, False, False),
    ("delta", "over capacity", "ERR_TOO_LARGE", TOO_LARGE_MSG, False, False),
    ("delta", "host_capacity", "ERR_TOO_LARGE", "rtx_update_delta: the stream is longer than host_capacity (the next call gives a key frame)", True, True),
    ("half", "mode -1", "ERR_INVALID_MODE", "rtx_update_half: not a character mode", False, True),
    ("half", "mode 6", "ERR_INVALID_MODE", "rtx_update_half: not a character mode", False, True),
    ("half", "SDL", "ERR_INVALID_MODE", "rtx_update_half: not a character mode", False, True),
    ("half", "x = 0", "ERR_INVALID_ARGUMENT", HALF_RANGE_MSG, False, True),
    ("half", "over capacity", "ERR_TOO_LARGE", HALF_LARGE_MSG, False, True),
    ("half", "host_capacity", "ERR_TOO_LARGE", "rtx_update_half: the stream is longer than host_capacity", True, True),
]


def test_the_refusal_table(R, pinned):
    mode = R.RGB_ASCII
    p = R.camera_params(CW, CH)
    with R.Context(CW, CH) as c:
        c.set_reference_default_scene()
        k = Caller(R, c, pinned)
        assert k.physics_agrees()
        for entry, case, status, message, stepped, key in REFUSALS:
            what = (entry, case)
            # a console of half the rows for the half-block calls: CW x CH pixels
            good = copy_params(R, p, y=CH // 2) if entry == "half" else p
            q, m, capacity = good, mode, 1 << 30
            if case.startswith("mode"):
                m = int(case.split()[1])
            elif case == "SDL":
                m = R.SDL
            elif case == "x = 0":
                q = copy_params(R, good, x=0)
            elif case == "over capacity":
                q = copy_params(R, good, y=int(good.y) + 1)
            else:
                assert case == "host_capacity"
                capacity = 8
            assert k.next_delta_kind(p, mode) in (R.DELTA_KEY, R.DELTA_DIFF)   # from here on the consumer shows this frame
            rc, msg = k.call(entry, q, m, capacity=capacity)
            assert (rc, msg) == (getattr(R, status), message), what
            if stepped:
                k.step_oracle()
            assert k.physics_agrees(), what
            assert k.next_delta_kind(p, mode) == (R.DELTA_KEY if key else R.DELTA_DIFF), what
            if entry == "begin":
                # both tickets are still to be had, and the frames under them are whole
                want = O.minimize(mode, O.render(U.oracle_params(p), k.sc, mode), CW, CH)
                tickets = []
                for dst in range(2):
                    rc, msg = k.call("begin", p, mode, physics=False, dst=dst)
                    assert rc == 0, (what, msg)
                    tickets.append(k.ticket.value)
                assert sorted(tickets) == [0, 1], what
                for dst, t in enumerate(tickets):
                    assert k.end(t)[0] == 0 and np.array_equal(pinned[dst][1][:k.n.value], want), what


def test_update_begin_with_both_slots_busy_and_update_end_on_an_idle_ticket(R, pinned):
    mode = R.BIT_PIXEL
    p = R.camera_params(CW, CH)
    with R.Context(CW, CH) as c:
        c.set_reference_default_scene()
        k = Caller(R, c, pinned)
        idle_msg = "rtx_update_end: no frame in flight under this ticket"
        assert k.next_delta_kind(p, mode) == R.DELTA_KEY
        for t in (0, 1):
            assert k.end(t) == (R.ERR_INVALID_ARGUMENT, idle_msg)
        assert k.next_delta_kind(p, mode) == R.DELTA_DIFF      # rtx_update_end hands nothing out
        tickets = []
        for dst in range(2):
            rc, msg = k.call("begin", p, mode, dst=dst)
            assert rc == 0, msg
            k.step_oracle()
            tickets.append((k.ticket.value, O.minimize(mode, O.render(U.oracle_params(p), k.sc, mode), CW, CH)))
        assert k.next_delta_kind(p, mode) == R.DELTA_KEY
        k.ticket.value = -7
        rc, msg = k.call("begin", p, mode)
        assert (rc, msg) == (R.ERR_INVALID_ARGUMENT, "rtx_update_begin: both slots are in flight; call rtx_update_end first")
        assert k.ticket.value == -7 and k.physics_agrees()     # no step, no ticket
        assert k.next_delta_kind(p, mode) == R.DELTA_KEY
        for dst, (t, want) in enumerate(tickets):
            assert k.end(t)[0] == 0 and np.array_equal(pinned[dst][1][:k.n.value], want), t
            assert k.end(t) == (R.ERR_INVALID_ARGUMENT, idle_msg)
        assert k.next_delta_kind(p, mode) == R.DELTA_DIFF


def test_the_next_delta_after_a_frame_of_another_entry_point_is_a_key_frame(R, pinned):
    mode = R.RGB_PIXEL
    p = R.camera_params(CW, CH)
    half = copy_params(R, p, y=CH // 2)
    with R.Context(CW, CH) as c:
        c.set_reference_default_scene()
        k = Caller(R, c, pinned)
        for entry in ("update", "begin", "half", "delta"):
            assert k.next_delta_kind(p, mode) in (R.DELTA_KEY, R.DELTA_DIFF)
            rc, msg = k.call(entry, half if entry == "half" else p, R.SDL if entry in ("update", "begin") else mode, physics=False)
            assert rc == 0, (entry, msg)
            if entry == "begin":
                assert k.end(k.ticket.value)[0] == 0
            assert k.next_delta_kind(p, mode) == (R.DELTA_DIFF if entry == "delta" else R.DELTA_KEY), entry


# ---- a mixed sequence

def oracle_words(p, sc, mode):
    """The oracle's frame as the pixel words the trace stores."""
    W, H = int(p.x), int(p.y)
    return U.records_to_words(O.render(U.oracle_params(p), sc, mode), W, H, 20)


def test_a_mixed_sequence_equals_the_oracle_frame_by_frame(R, pinned):
    mode = R.RGB_ASCII
    p = R.camera_params(CW, CH)
    with R.Context(CW, 2 * CH) as c:      # (the half-block frame samples CW x 2 CH pixels)
        c.set_reference_default_scene()
        k = Caller(R, c, pinned)

        def stepped_stream():
            k.step_oracle()
            return O.minimize(mode, O.render(U.oracle_params(p), k.sc, mode), CW, CH)

        def got(dst=0):
            return pinned[dst][1][:k.n.value]

        def ok(r):
            assert r[0] == 0, r[1]

        ok(k.call("update", p, mode))                                   # 1 blocking
        assert np.array_equal(got(), stepped_stream())
        ok(k.call("begin", p, mode, dst=0))                             # 2 begin
        ta, want_a = k.ticket.value, stepped_stream()
        ok(k.call("begin", p, mode, dst=1))                             # 3 begin
        tb, want_b = k.ticket.value, stepped_stream()
        ok(k.end(ta))                                                   # 4 end
        assert np.array_equal(got(0), want_a)
        ok(k.call("delta", p, mode, dst=0))                             # 5 delta: a key frame
        assert k.kind.value == R.DELTA_KEY and np.array_equal(got(0), stepped_stream())
        ok(k.end(tb))                                                   # 6 end: the frame begun before the delta
        assert np.array_equal(got(1), want_b)
        ok(k.call("half", p, mode))                                     # 7 half
        k.step_oracle()
        assert bytes(got()) == RH.half_stream(mode, CW, CH, oracle_words(copy_params(R, p, y=2 * CH), k.sc, mode))
        ok(k.call("delta", p, mode))                                    # 8 delta: a key frame again
        assert k.kind.value == R.DELTA_KEY and np.array_equal(got(), stepped_stream())
        before = oracle_words(p, k.sc, mode)
        ok(k.call("delta", p, mode))                                    # and the one after it is a delta against frame 8
        k.step_oracle()
        want, cells, _ = RD.delta_stream(mode, CW, CH, oracle_words(p, k.sc, mode), before)
        assert k.kind.value == R.DELTA_DIFF and cells > 0 and bytes(got()) == want
        assert k.physics_agrees()
        assert (c.get_option(R.STAT_DELTA_FRAMES), c.get_option(R.STAT_DELTA_KEYFRAMES), c.get_option(R.STAT_HALF_FRAMES)) == (3, 2, 1)
