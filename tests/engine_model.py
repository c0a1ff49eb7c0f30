"""A CPU model of what a caller can observe of one engine (include/mpimodel.h), and the
scripts that drive an engine and the model side by side over a long life.

Helper module: not collected by pytest. tests/test_engine_model_cpu.py checks the model
itself, tests/test_gpu_lifetime.py compares engines with it.

The model: per attribute one numpy field (the whole H x W grid) and an optional rate field,
the flow list, steps_done and the history of step sums. Its semantics are the header's, not
the engine's code: one step applies the flows in declared order (the oracle's program step
for runs of diffusions and transfers, its general step with outf = f * v for a rate-field
diffusion); fill / upload reset steps_done and nothing else; run(n, r) appends the sums after
every step s of (steps_done, steps_done + n] with s % r == 0; prepare and set_timing change
nothing.

A script is a list of (method, args) tuples with mpimodel.Engine's method names and
positional arguments. Three placeholders keep a script printable and independent of the
grid: ("state", seed) is fill_random's field for that seed, ("field", seed, nrows) the first
nrows rows of random_field for that seed, and a `captured` of None in point_apply is the
model's current value of the source cell. materialize() turns them into call arguments.
"""
import math

import numpy as np

from test_gpu_ratefield import neighbour_counts, random_field

SEED = 0x4D50494D
DIFFUSE, TRANSFER, DIFFUSE_FIELD = 1, 2, 3
FILL_UNIFORM, FILL_RANDOM = 0, 1

RUN_LENGTHS = (1, 2, 3, 7, 8, 16, 17, 32, 40, 45)
REDUCE_EVERY = (0, 1, 2, 3, 5)
SEEDS = range(8)
N_OPS = 24

# ops that change what download / sums / sums_history return, or the program
STATE_OPS = {"fill", "fill_random", "upload", "clear_flows", "add_diffuse", "add_transfer",
             "add_diffuse_field", "rate_field_upload", "rate_field_fill", "point_apply", "run",
             "clear_history"}
PROGRAM_OPS = {"clear_flows", "add_diffuse", "add_transfer", "add_diffuse_field"}
# ops that change nothing observable
HINT_OPS = {"prepare", "set_timing"}

# creation-time environments and the smallest grids that reach each kernel family:
# (n_attr, environment, (H, W))
CONFIGS_1 = [
    (1, {}, (27, 257)),                                         # small-slab wide kernel
    (1, {"MM_WIDE": 0, "MM_SEG_WAVES": 64}, (50, 257)),         # mm_passk_kernel, 16-row segments
    (1, {"MM_WIDE": 1, "MM_STEPS_PER_PASS": 20}, (37, 130)),    # K = 20 wide kernel
    (1, {"MM_PASSK": 0, "MM_ROWS_PER_WAVE": 16}, (67, 300)),    # one-step kernel, 16-row blocks
    (1, {"MM_FIELD_STEPS": 4, "MM_SEG_WAVES": 64}, (50, 257)),  # mm_fieldk_kernel, K = 4
    (1, {"MM_FIELD_STEPS": 3}, (27, 257)),                      # fused field passes, odd flips
    (1, {"MM_GRAPH": 0}, (27, 257)),                            # eager path only
    (1, {"MM_GRAPH_MAX_LAUNCHES": 3}, (27, 257)),               # short graphs
]
CONFIGS_3 = [(3, {}, (27, 257)), (3, {"MM_WIDE": 0}, (27, 257))]
CONFIGS_4 = [(4, env, shape)
             for env in ({}, {"MM_CHAIN_RING": 0}, {"MM_STEPS_PER_PASS": 4})
             for shape in ((37, 130), (67, 301))]
CONFIGS = CONFIGS_1 + CONFIGS_3 + CONFIGS_4


def config_id(cfg):
    n_attr, env, (H, W) = cfg
    e = ",".join(f"{k[3:]}={v}" for k, v in env.items()) or "default"
    return f"a{n_attr}-{e}-{H}x{W}"


class ModelError(AssertionError):
    """A script asked the model for something the engine would refuse."""


class EngineModel:
    def __init__(self, O, H, W, n_attr=1):
        self.O, self.H, self.W, self.n_attr = O, H, W, n_attr
        self.v = [np.zeros((H, W)) for _ in range(n_attr)]  # device buffers start zeroed
        self.f = [None] * n_attr
        self.flows = []
        self.steps_done = 0
        self.hist = []
        self.cnt = neighbour_counts(H, W)

    def _attr(self, a):
        if not 0 <= a < self.n_attr:
            raise ModelError(f"attribute {a} out of range")

    # ---- state ---------------------------------------------------------------------------
    def fill(self, attr=0, mode=FILL_UNIFORM, value=1.0, seed=SEED):
        self._attr(attr)
        if mode == FILL_RANDOM:
            self.v[attr] = self.O.fill_random(self.H, self.W, seed=seed)
        else:
            self.v[attr] = np.full((self.H, self.W), float(value))
        self.steps_done = 0

    def fill_random(self, attr=0, seed=SEED):
        self.fill(attr, FILL_RANDOM, 0.0, seed)

    def upload(self, host, attr=0):
        self._attr(attr)
        a = np.array(host, dtype=np.float64)
        assert a.shape == (self.H, self.W)
        self.v[attr] = a
        self.steps_done = 0

    def download(self, attr=0):
        return self.v[attr].copy()

    def point_apply(self, sx, sy, captured, rate, attr=0):
        self._attr(attr)
        self.v[attr] = self.O.point_apply(self.v[attr], sx, sy, captured, rate)

    # ---- program -------------------------------------------------------------------------
    def clear_flows(self):
        self.flows = []

    def add_diffuse(self, attr, rate):
        self._attr(attr)
        self.flows.append((DIFFUSE, attr, attr, float(rate)))

    def add_transfer(self, a, b, rate):
        self._attr(a)
        if b >= self.n_attr:
            raise ModelError(f"target attribute {b} out of range")
        self.flows.append((TRANSFER, a, -1 if b < 0 else b, float(rate)))

    def add_diffuse_field(self, attr):
        self._attr(attr)
        self.flows.append((DIFFUSE_FIELD, attr, attr, 0.0))

    # ---- rate fields ---------------------------------------------------------------------
    def rate_field_upload(self, host, attr=0, row0=0):
        """Rows row0.. of the GLOBAL grid (the model is one slab: local = global); rows outside
        the grid are skipped, rows never uploaded are 0."""
        self._attr(attr)
        a = np.asarray(host, dtype=np.float64)
        assert a.ndim == 2 and a.shape[1] == self.W
        if self.f[attr] is None:
            self.f[attr] = np.zeros((self.H, self.W))
        lo, hi = max(row0, 0), min(row0 + a.shape[0], self.H)
        if hi > lo:
            self.f[attr][lo:hi] = a[lo - row0:hi - row0]

    def rate_field_fill(self, value, attr=0):
        self._attr(attr)
        self.f[attr] = np.full((self.H, self.W), float(value))

    # ---- running -------------------------------------------------------------------------
    def step(self):
        O, run = self.O, []

        def flush():
            if run:
                self.v = self.O.program_step(self.v, run)
                del run[:]

        for fl in self.flows:
            if fl[0] == DIFFUSE_FIELD:
                flush()
                a = fl[1]
                v = self.v[a]
                self.v[a] = O.field_step_general(v, np.where(self.cnt > 0, self.f[a] * v, 0.0))
            else:
                run.append(fl)
        flush()

    def run(self, nsteps, reduce_every=0):
        if nsteps < 0 or reduce_every < 0:
            raise ModelError("run: bad arguments")
        if nsteps == 0:
            return
        if not self.flows:
            raise ModelError("run: no flow")
        for fl in self.flows:
            if fl[0] == DIFFUSE_FIELD and self.f[fl[1]] is None:
                raise ModelError(f"run: attribute {fl[1]} has no rate field")
        for s in range(self.steps_done + 1, self.steps_done + nsteps + 1):
            self.step()
            if reduce_every > 0 and s % reduce_every == 0:
                self.hist.append(self.sums())
        self.steps_done += nsteps

    def prepare(self, nsteps, reduce_every=0):
        pass

    def set_timing(self, on):
        pass

    # ---- sums ----------------------------------------------------------------------------
    def sums(self):
        return [math.fsum(v.ravel()) for v in self.v]

    def sums_history(self):
        return np.array(self.hist, dtype=np.float64).reshape(len(self.hist), self.n_attr)

    def clear_history(self):
        self.hist = []

    def info(self):
        return {"steps_done": self.steps_done, "hist_entries": len(self.hist)}

    def field_attrs(self):
        return [a for a in range(self.n_attr) if self.f[a] is not None]


def materialize(method, args, model):
    """The call arguments of a script entry: placeholders resolved against the model."""
    args = list(args)
    for i, x in enumerate(args):
        if isinstance(x, tuple) and x and x[0] == "state":
            args[i] = model.O.fill_random(model.H, model.W, seed=x[1])
        elif isinstance(x, tuple) and x and x[0] == "field":
            args[i] = random_field(model.H, model.W, seed=x[1])[:x[2]]
        elif isinstance(x, tuple) and x and x[0] == "nanfield":
            args[i] = np.zeros((x[1], model.W))
            args[i][-1, -1] = float("nan")
    if method == "point_apply" and args[2] is None:
        attr = args[4] if len(args) > 4 else 0
        args[2] = float(model.v[attr][args[0], args[1]])
    return args


def apply_op(target, method, args):
    getattr(target, method)(*args)


# Two entries that are no Engine method: ("refuse", (method, args)) is a call the engine must
# refuse with MMError and that leaves no trace (the model skips it); ("cached_run", (n, r)) is
# a run whose graphs exist already, so it must instantiate none (the model runs it).
REFUSE, CACHED_RUN = "refuse", "cached_run"


def run_model(O, cfg, script, each=None):
    """The script on the model alone; each(i, model) after every entry."""
    n_attr, _, (H, W) = cfg
    m = EngineModel(O, H, W, n_attr)
    for i, (method, args) in enumerate(script):
        if method == CACHED_RUN:
            m.run(*args)
        elif method != REFUSE:
            apply_op(m, method, materialize(method, args, m))
        if each:
            each(i, m)
    return m


def format_script(script):
    return "[\n" + "".join(f"    {op!r},\n" for op in script) + "]"


# ---- programs ------------------------------------------------------------------------------
def program(flows, clear=True):
    """Script entries that set a program: [(kind, a, b, rate)] as oracle.program_step takes
    them, kind 3 a rate-field diffusion of a."""
    out = [("clear_flows", ())] if clear else []
    for kind, a, b, r in flows:
        if kind == DIFFUSE:
            out.append(("add_diffuse", (a, r)))
        elif kind == TRANSFER:
            out.append(("add_transfer", (a, b, r)))
        else:
            out.append(("add_diffuse_field", (a,)))
    return out


def D(a, r):
    return (DIFFUSE, a, a, r)


def T(a, b, r):
    return (TRANSFER, a, b, r)


def F(a):
    return (DIFFUSE_FIELD, a, a, 0.0)


RING = [T(0, 1, 0.05), T(1, 2, 0.03), T(2, 3, 0.02), T(3, 0, 0.01),
        D(0, 0.1), D(1, 0.1), D(2, 0.05), D(3, 0.2)]  # tests/test_gpu_padding.py's C5_FLOWS


def fills(n_attr, seed=SEED):
    return [("fill_random", (a, seed + a)) for a in range(n_attr)]


# ---- hand-written lifetimes (tests/test_gpu_lifetime.py runs them on the GPU) ---------------
def script_aba(n_attr, H, W):
    """a. Program A, then B, then A again, the state carried over; then a refill and A."""
    if n_attr == 1:
        A = [D(0, 0.1)]
        progs = [A, [D(0, 0.25)], A, [T(0, -1, 0.05), D(0, 0.1)], A, [D(0, 0.1), D(0, 0.2)],
                 [F(0)], A, [F(0), D(0, 0.15)], A]
    elif n_attr == 4:
        A = RING
        long_pre = [T(0, 1, 0.05), T(1, 2, 0.03), T(2, 3, 0.02), T(3, 0, 0.01), T(0, 2, 0.04),
                    T(1, 3, 0.02), D(0, 0.1), D(2, 0.2)]  # pre-chain of 6 > kMaxChain = 4
        progs = [A, RING + [T(3, -1, 0.02)], [D(0, 0.1)], A, [D(1, 0.2), D(3, 0.05)],
                 [T(0, 2, 0.1), D(0, 0.1), D(1, 0.1), D(2, 0.3)],
                 [T(0, 1, 0.1), T(2, 3, 0.2), T(3, -1, 0.01)], long_pre, A]
    else:
        A = [T(0, 1, 0.05), D(1, 0.1), D(2, 0.2)]
        progs = [A, [D(0, 0.3)], A, [F(1), D(0, 0.1)], [T(2, 0, 0.1), T(0, -1, 0.02)], A]
    s = fills(n_attr)
    for a in range(n_attr):
        s.append(("rate_field_upload", (("field", 7 + a, H), a, 0)))
    lens = (17, 8, 3, 16, 7, 2, 40, 1, 32, 45)
    for i, p in enumerate(progs):
        s += program(p)
        # the same run twice under every program: its graph key exists at either parity when
        # the next program arrives; then a run of its own
        s += [("run", (16, 0)), ("run", (16, 0))]
        s.append(("run", (lens[i % len(lens)], REDUCE_EVERY[i % len(REDUCE_EVERY)])))
    s += fills(n_attr) + program(A) + [("run", (17, 2))]
    return s, A


def script_incremental(n_attr, H, W):
    """b. add_* after a run, without clear_flows: the one-pass K-step program becomes a
    multi-pass one-step program in mid-life, and grows further."""
    # Before every add_* the same run twice, after it the same run again, at the same
    # reduction phase: the graph of that key exists at either parity, and replaying it would
    # run the program as it was before the add.
    last = n_attr - 1
    s = fills(n_attr) + program([D(0, 0.1)], clear=False)
    s += [("run", (16, 2)), ("run", (16, 2))]
    s += program([D(last, 0.2)], clear=False) + [("run", (16, 2)), ("run", (7, 0)), ("run", (17, 2))]
    s += [("run", (8, 1)), ("run", (8, 1))]
    s += program([T(0, last if last else -1, 0.05)], clear=False) + [("run", (8, 1)), ("run", (3, 1))]
    s += [("run", (32, 0)), ("run", (32, 0)), ("rate_field_fill", (0.125, last))]
    s += program([F(last)], clear=False) + [("run", (32, 0)), ("run", (7, 3)), ("run", (16, 0))]
    return s


def script_fields(n_attr, H, W):
    """c. Rate fields over a lifetime."""
    b = n_attr - 1
    s = fills(n_attr) + [("rate_field_upload", (("field", 7, H), 0, 0))]
    s += program([F(0)], clear=False) + [("run", (17, 1)), ("run", (8, 0))]
    # a few rows again, from another field; rows above the grid are skipped
    s += [("rate_field_upload", (("field", 11, 5), 0, 9)), ("run", (16, 0)),
          ("rate_field_upload", (("field", 13, 4), 0, -2)), ("run", (3, 2)),
          ("rate_field_upload", (("field", 17, 3), 0, H - 3)), ("run", (8, 0))]
    s += [("rate_field_fill", (0.2, 0)), ("run", (17, 5))]
    # two programs without the field, then the field of two programs ago once more
    s += program([D(0, 0.1)]) + [("run", (16, 0))]
    s += program([T(0, -1, 0.01), D(0, 0.3)]) + [("run", (7, 1))]
    s += program([F(0)]) + [("run", (8, 0)), ("run", (8, 0))]
    if n_attr > 1:
        # the first field of another attribute arrives after graphs exist
        s += [("rate_field_upload", (("field", 19, H), b, 0))]
        s += program([F(b)], clear=False) + [("run", (16, 0)), ("run", (17, 2))]
    else:
        s += program([F(0)], clear=False) + [("run", (16, 0)), ("run", (17, 2))]
    return s


def script_reductions(n_attr, H, W):
    """d. reduce_every changes between runs (the phase comes from steps_done), clear_history
    between replays of one cached graph, a fill of one attribute resets the phase for all."""
    flows = [D(0, 0.1)] if n_attr == 1 else [T(0, 1, 0.05)] + [D(a, 0.1) for a in range(n_attr)]
    s = fills(n_attr) + program(flows, clear=False)
    s += [("run", (7, 3)), ("run", (8, 3)), ("run", (16, 5)), ("run", (3, 2)), ("run", (17, 2))]
    s += [("run", (16, 2)), ("clear_history", ()), ("run", (16, 2)), ("run", (16, 2)),
          ("clear_history", ()), ("run", (16, 2))]
    s += [("run", (3, 0)), ("fill_random", (n_attr - 1, SEED + 9)), ("run", (16, 2)),
          ("run", (7, 5)), ("fill", (0, FILL_UNIFORM, 1.5, 0)), ("run", (8, 5)), ("run", (45, 1))]
    return s


def script_history_growth(n_attr, H, W):
    """d. Past the initial history capacity of 4096 entries once."""
    s = fills(n_attr) + program([D(0, 0.1)], clear=False)
    s += [("run", (32, 1))] * 127 + [("run", (45, 1))]  # 4109 entries
    return s


def script_prepare(n_attr, H, W):
    """e. prepare(n, r), a run of another length, then the prepared one."""
    flows = [D(0, 0.1)] if n_attr == 1 else \
        [T(a, (a + 1) % n_attr, 0.02) for a in range(n_attr)] + [D(a, 0.1) for a in range(n_attr)]
    s = fills(n_attr) + program(flows, clear=False)
    s += [("prepare", (32, 2)), ("run", (7, 2)), ("run", (32, 2)), ("prepare", (45, 0)),
          ("prepare", (16, 1)), ("run", (16, 1)), ("run", (45, 0)), ("run", (32, 2))]
    return s


def script_points(n_attr, H, W):
    """f. point_apply between runs without a read, on odd and on even parity."""
    a = n_attr - 1
    s = fills(n_attr) + program([D(a, 0.1)], clear=False)
    s += [("run", (1, 0)), ("point_apply", (3, 5, None, 0.5, a)), ("run", (16, 0)),
          ("point_apply", (0, 0, None, 0.3, a)), ("run", (3, 1)),
          ("point_apply", (H - 1, W - 1, None, 0.25, a)), ("point_apply", (H // 2, 0, None, 0.1, 0)),
          ("run", (17, 0)), ("point_apply", (H - 1, 128, None, 0.5, a)), ("run", (8, 2)),
          ("run", (7, 0)), ("point_apply", (13, W - 2, None, 0.4, a)), ("run", (32, 0))]
    return s


def script_refusals(n_attr, H, W):
    """g. Calls that must fail, between the steps of a life: argument errors the engine rejects
    on the host before any launch. The same run twice first, so that its graph exists at
    either buffer parity; the run after the refusals must then find it."""
    a = n_attr - 1
    nan = float("nan")
    bad_args = [
        ("add_diffuse", (0, nan)), ("add_diffuse", (n_attr, 0.1)), ("add_diffuse", (-1, 0.1)),
        ("add_transfer", (0, n_attr, 0.1)), ("add_diffuse_field", (n_attr,)),
        ("rate_field_upload", (("nanfield", 3), a, 2)),
        ("rate_field_upload", (("field", 7, 2), a, H + 19)),
        ("rate_field_upload", (("field", 7, 1), a, -21)),
        ("rate_field_upload", (("field", 7, H), n_attr, 0)),
        ("rate_field_fill", (nan, a)), ("rate_field_fill", (0.1, n_attr)),
        ("run", (-1, 0)), ("run", (8, -1)), ("prepare", (-1, 0)),
        ("point_apply", (H, 0, 1.0, 0.1, 0)), ("fill", (n_attr, FILL_UNIFORM, 1.0, 0)),
    ]
    refused = [(REFUSE, b) for b in bad_args]
    s = fills(n_attr) + program([D(a, 0.1)], clear=False)
    s += [("run", (16, 0)), ("run", (16, 0))] + refused + [(CACHED_RUN, (16, 0)), ("run", (7, 1))]
    # a field program whose attribute has no field: refused until the field arrives
    s += program([F(a)]) + [(REFUSE, ("run", (8, 0))), (REFUSE, ("prepare", (8, 0))),
                            (REFUSE, ("rate_field_upload", (("nanfield", 1), a, 0))),
                            (REFUSE, ("run", (1, 1)))]
    s += [("rate_field_upload", (("field", 7, H), a, 0)), ("run", (8, 0)), ("run", (8, 0))]
    s += refused + [(CACHED_RUN, (8, 0)), ("run", (17, 2))]
    return s


def script_timing(n_attr, H, W):
    """e. set_timing(True), a run, timing(), set_timing(False), a run; the test reads timing()
    after entry TIMED_RUN, counted from the end."""
    flows = [D(0, 0.1)] if n_attr == 1 else \
        [T(a, (a + 1) % n_attr, 0.02) for a in range(n_attr)] + [D(a, 0.1) for a in range(n_attr)]
    s = fills(n_attr) + program(flows, clear=False)
    s += [("run", (7, 0)), ("set_timing", (True,)), ("run", (17, 2)), ("set_timing", (False,)),
          ("run", (17, 2)), ("run", (16, 0))]
    return s


TIMED_RUN = -4

CHAIN_SHAPES = [(77, 300, 4), (27, 257, 3)]
CHAIN_ENV = {"MM_WIDE": 0, "MM_STEPS_PER_PASS": 5}


def script_chain(n_attr, H, W):
    """h. A host-transport chain reprogrammed in lockstep (the model is the whole grid; the
    test hands every slab its rows of a field upload and exchanges the halos of a run)."""
    s = fills(1) + program([D(0, 0.1)], clear=False) + [("run", (16, 1))]
    s += program([F(0)]) + [("rate_field_upload", (("field", 7, H), 0, 0)), ("run", (7, 1))]
    s += program([D(0, 0.3)]) + [("run", (8, 1))]
    return s


# what the runner of tests/test_gpu_lifetime.py calls beside the script's own methods
RUNNER_CALLS = ("info", "download", "sums", "sums_history", "synchronize", "pass_plan",
                "pass_kernel", "timing")
# Engine method -> the entry point of include/mpimodel.h behind it
EXPORT_OF = {"info": "mm_engine_info", "fill": "mm_fill", "fill_random": "mm_fill",
             "upload": "mm_upload", "download": "mm_download", "clear_flows": "mm_clear_flows",
             "add_diffuse": "mm_add_flow", "add_transfer": "mm_add_flow",
             "add_diffuse_field": "mm_add_flow", "rate_field_upload": "mm_rate_field_upload",
             "rate_field_fill": "mm_rate_field_fill", "point_apply": "mm_point_apply",
             "run": "mm_run", "prepare": "mm_prepare", "pass_plan": "mm_pass_plan",
             "pass_kernel": "mm_pass_kernel", "synchronize": "mm_synchronize", "sums": "mm_sums",
             "sums_history": "mm_sums_history", "clear_history": "mm_clear_history",
             "set_timing": "mm_set_timing", "timing": "mm_timing"}
# entry points no lifetime script calls, each with the reason
NOT_SEQUENCED = {
    "mm_abi_version": "host-only helper",
    "mm_last_error": "host-only helper (the text of every MMError)",
    "mm_step_count": "host-only helper",
    "mm_partition_reference": "host-only helper",
    "mm_owner_reference": "host-only helper",
    "mm_partition_rows": "host-only helper (slabs of the chain scenario)",
    "mm_neighbor_count": "host-only helper",
    "mm_partition_rect_reference": "host-only helper",
    "mm_owner_rect_reference": "host-only helper",
    "mm_point_strict_applies": "host-only helper",
    "mm_wire_format_partition": "host-only helper",
    "mm_wire_format_flow": "host-only helper",
    "mm_wire_parse_partition": "host-only helper",
    "mm_wire_parse_flow": "host-only helper",
    "mm_point_apply_strict": "mm_point_apply behind the host-only predicate mm_point_strict_applies",
    "mm_comm_id_size": "RCCL bootstrap",
    "mm_comm_id_create": "RCCL bootstrap",
    "mm_device_count": "device query of the gpu fixture, no engine state",
    "mm_device_synchronize": "device-wide wait, no engine state",
    "mm_engine_create": "the start of every lifetime",
    "mm_engine_destroy": "the end of every lifetime",
    "mm_halo_export_rows": "halo transport: the chain scenario calls it around every pass",
    "mm_halo_import_rows": "halo transport: the chain scenario calls it around every pass",
    "mm_halo_export": "halo transport, one-row form of mm_halo_export_rows",
    "mm_halo_import": "halo transport, one-row form of mm_halo_import_rows",
    "mm_debug_read_rows": "debug hook",
    "mm_debug_fill_padding": "debug hook",
}


def all_scripts():
    """Every script the GPU tests run: (id, cfg, script). The environment does not reach the
    model, so one configuration per (n_attr, grid) stands for all of them."""
    seen, out = set(), []
    for cfg in CONFIGS:
        n_attr, _, (H, W) = cfg
        if (n_attr, H, W) in seen:
            continue
        seen.add((n_attr, H, W))
        for name, make in SCRIPTED.items():
            out.append((f"{name}-a{n_attr}-{H}x{W}", cfg, make(n_attr, H, W)))
        for seed in SEEDS:
            out.append((f"seed{seed}-a{n_attr}-{H}x{W}", cfg, random_script(cfg, seed)))
    out.append(("history-growth", CONFIGS_1[0], script_history_growth(1, *CONFIGS_1[0][2])))
    for H, W, _ in CHAIN_SHAPES:
        out.append((f"chain-{H}x{W}", (1, CHAIN_ENV, (H, W)), script_chain(1, H, W)))
    return out


SCRIPTED = {"aba": lambda n, H, W: script_aba(n, H, W)[0], "incremental": script_incremental,
            "fields": script_fields, "reductions": script_reductions, "prepare": script_prepare,
            "timing": script_timing, "points": script_points, "refusals": script_refusals}


# ---- seeded random scripts -------------------------------------------------------------------
def _rate(rng, hi=0.5):
    return float(np.round(rng.uniform(0.0, hi), 3))


def _trate(rng):
    return float(np.round(rng.uniform(0.001, 0.3), 3))  # (0, 0.3]


def _gen_program(rng, n_attr):
    """A random flow list: 1..3 flows for one attribute, up to 6 (or the ring) for several."""
    if n_attr == 4 and rng.random() < 0.3:
        return list(RING)
    flows = []
    for _ in range(int(rng.integers(1, 4 if n_attr == 1 else 7))):
        flows.append(_gen_flow(rng, n_attr))
    if not any(f[0] != TRANSFER for f in flows) and rng.random() < 0.7:
        flows.append(D(int(rng.integers(n_attr)), _rate(rng)))
    return flows


def _gen_flow(rng, n_attr):
    a = int(rng.integers(n_attr))
    kind = rng.choice([DIFFUSE, TRANSFER, DIFFUSE_FIELD], p=[0.5, 0.3, 0.2])
    if kind == DIFFUSE:
        return D(a, _rate(rng))
    if kind == DIFFUSE_FIELD:
        return F(a)
    b = -1 if n_attr == 1 else int(rng.choice([x for x in range(-1, n_attr) if x != a]))
    return T(a, b, _trate(rng))


def gen_script(rng, n_attr, n_ops=N_OPS):
    """A random lifetime of n_ops ops after the set-up (a fill_random per attribute and the
    first program). An op is one draw: a run, a program change (clear_flows and the new
    program's add_* calls, or one add_* without clear_flows), a state op (fill, fill_random,
    upload), a field op (rate_field_upload whole or of a few rows, rate_field_fill), a
    point_apply, a clear_history or a hint (prepare, set_timing). Every script holds 2..4
    program changes, 6..10 runs and at least one op of each other class, in random order. A
    program with a field diffusion is preceded by a field op for every attribute that has no
    field yet, so no script holds a call the engine refuses. Grid-independent: rows and
    columns of point sources and partial uploads are fractions resolved by grid_script()."""
    have = set()

    def need_fields(flows):
        out = []
        for f in flows:
            if f[0] == DIFFUSE_FIELD and f[1] not in have:
                have.add(f[1])
                out.append(("rate_field_upload", (("field", int(rng.integers(100)), "H"), f[1], 0)))
        return out

    classes = ["program"] * 2 + ["run"] * 6 + ["state", "field", "point", "history", "hint"]
    pool, weight = ["program", "run", "state", "field", "point", "history", "hint"], \
        [0.12, 0.3, 0.1, 0.16, 0.12, 0.08, 0.12]
    while len(classes) < n_ops:
        c = str(rng.choice(pool, p=weight))
        if classes.count(c) >= {"program": 4, "run": 10}.get(c, n_ops):
            continue
        classes.append(c)
    classes = [classes[i] for i in rng.permutation(len(classes))]

    flows = _gen_program(rng, n_attr)
    s = fills(n_attr) + need_fields(flows) + program(flows, clear=False)
    timing = False
    last_run, repeat = None, False
    prev = "program"
    for c in classes:
        after_program, prev = prev == "program", c
        if c == "run":
            # half of the runs repeat the run before: the same graph key (at the same phase),
            # whatever happened to the fields, the state and the history in between; so does
            # the first run after an add_* without clear_flows
            if last_run is None or not (repeat or rng.random() < 0.5):
                last_run = (int(rng.choice(RUN_LENGTHS)), int(rng.choice(REDUCE_EVERY)))
            repeat = False
            s.append(("run", last_run))
        elif c == "program":
            # (an add_* right after another program change would be part of that change)
            if rng.random() < 0.3 and len(flows) < 8 and not after_program:  # incremental
                new = [_gen_flow(rng, n_attr)]
                flows = flows + new
                s += need_fields(new) + program(new, clear=False)
                repeat = True
            else:
                flows = _gen_program(rng, n_attr)
                s += need_fields(flows) + program(flows)
        elif c == "state":
            a, k = int(rng.integers(n_attr)), int(rng.integers(3))
            if k == 0:
                s.append(("fill_random", (a, SEED + int(rng.integers(1000)))))
            elif k == 1:
                s.append(("upload", (("state", SEED + int(rng.integers(1000))), a)))
            else:
                s.append(("fill", (a, FILL_UNIFORM, float(np.round(rng.uniform(1.0, 2.0), 3)), 0)))
        elif c == "field":
            a, k = int(rng.integers(n_attr)), int(rng.integers(3))
            have.add(a)
            if k == 0:
                s.append(("rate_field_upload", (("field", int(rng.integers(100)), "H"), a, 0)))
            elif k == 1:  # a few rows at a fraction of the height, or hanging over the top
                s.append(("rate_field_upload", (("field", int(rng.integers(100)), int(rng.integers(1, 6))),
                                                a, ("row", float(np.round(rng.uniform(-0.05, 0.8), 3))))))
            else:
                s.append(("rate_field_fill", (_rate(rng), a)))
        elif c == "point":
            s.append(("point_apply", (("row", float(np.round(rng.random(), 3))),
                                      ("col", float(np.round(rng.random(), 3))), None,
                                      _rate(rng), int(rng.integers(n_attr)))))
        elif c == "history":
            s.append(("clear_history", ()))
        else:
            if rng.random() < 0.5:
                s.append(("prepare", (int(rng.choice(RUN_LENGTHS)), int(rng.choice(REDUCE_EVERY)))))
            else:
                timing = not timing
                s.append(("set_timing", (timing,)))
    return s


def grid_script(script, H, W):
    """gen_script's fractions as rows and columns of an H x W grid."""
    def fix(x):
        if isinstance(x, tuple) and x and x[0] == "row":
            return min(H - 1, int(x[1] * H)) if x[1] >= 0 else -2
        if isinstance(x, tuple) and x and x[0] == "col":
            return min(W - 1, int(x[1] * W))
        if isinstance(x, tuple) and x and x[0] == "field" and x[2] == "H":
            return ("field", x[1], H)
        return x
    return [(m, tuple(fix(x) for x in args)) for m, args in script]


def random_script(cfg, seed):
    n_attr, _, (H, W) = cfg
    rng = np.random.default_rng([seed, n_attr])
    return grid_script(gen_script(rng, n_attr), H, W)


def op_class(method):
    return {"run": "run", "fill": "state", "fill_random": "state", "upload": "state",
            "rate_field_upload": "field", "rate_field_fill": "field", "point_apply": "point",
            "clear_history": "history", "prepare": "hint", "set_timing": "hint"}.get(method, "program")
