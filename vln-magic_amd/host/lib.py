"""ctypes binding of libmagic_hip.so.  The signature table and the descriptor structs are not written here: host/abi.py reads them
from include/magic_hip.h, the one definition of the C ABI (the kernels include the same file).

The product path has NO CPU fallback: if the library is missing or a kernel returns an error code the
call raises.  Tensors are passed as raw device pointers; the stream is torch's current HIP stream.
"""
import ctypes as C
import os
import threading

import torch

from . import abi

_HERE = os.path.dirname(os.path.abspath(__file__))
# MAGIC_LIB_FILE: load another build of the library (same-box A/B of a kernel change: `MAGIC_LIB_FILE=.../libmagic_hip_prev.so
# MAGIC_ALLOW_STALE_LIB=1 python bench.py ...`); the build-id check still runs against whatever is loaded
LIB_PATH = os.environ.get("MAGIC_LIB_FILE") or os.path.join(os.path.dirname(_HERE), "libmagic_hip.so")

vp, i32, i64, f32, u32, u64 = C.c_void_p, C.c_int, C.c_longlong, C.c_float, C.c_uint, C.c_ulonglong


class MagicHipError(RuntimeError):
    pass


# The ABI tables come from the header itself (host/abi.py reads it once per process): SIGNATURES = entry point -> argument ctypes, STRUCTS =
# header struct name -> ctypes.Structure class, fields named as in C.  A missing or unreadable header is as fatal as a missing library.
try:
    SIGNATURES, STRUCTS = abi.load()
except (OSError, ValueError) as e:
    raise MagicHipError(f"{abi.HEADER}: the C ABI header cannot be read ({e}); the binding has no other table") from e

DwDesc = STRUCTS["magic_dw_desc"]
DwCatProb = STRUCTS["magic_dwcat_prob"]
MseDesc = STRUCTS["magic_mse_desc"]
NodeIn = STRUCTS["magic_node_in"]
DropD = STRUCTS["magic_drop_desc"]
PanoIn = STRUCTS["magic_pano_in"]
LnIn = STRUCTS["magic_ln_in"]
PanoInBwd = STRUCTS["magic_pano_in_bwd"]
LnBwdIn = STRUCTS["magic_ln_bwd_in"]
CsrProb = STRUCTS["magic_csr_prob"]
SkbProb = STRUCTS["magic_skb_prob"]
EncLayer = STRUCTS["magic_enc_layer"]
EncSeg = STRUCTS["magic_enc_seg"]
EncParams = STRUCTS["magic_enc_params"]
SapLossParams = STRUCTS["magic_sap_loss_params"]
ChainParams = STRUCTS["magic_chain_params"]
XLayer = STRUCTS["magic_xenc_layer"]
XSeg = STRUCTS["magic_xenc_seg"]
XParams = STRUCTS["magic_xenc_params"]
RbwSeg = STRUCTS["magic_rowbwd_seg"]
RbwParams = STRUCTS["magic_rowbwd_params"]


def _ptrs(cls):
    """the pointer members of a struct, in order"""
    return tuple(n for n, t in cls._fields_ if t is vp)


XL_PTRS = _ptrs(XLayer)
# magic_rowbwd_seg's pointer members in three groups, because ops.rowbwd fills them under different conditions (literals: a group is not
# "the pointer members of X"; together they are, which is checked): the per-token chain, always; the in-launch attention backward
# (round 6), mode != 0; the map encoder's graph-distance bias, whose two gradients come out of that attention backward
RBW_PTRS = ("dqkv_n", "WqkvT_n", "dao_n", "dfo_in", "dfod_in", "y2", "rstd2", "g2", "b2", "dg2", "db2", "z", "W2T", "W1T",
            "y1", "rstd1", "g1", "b1", "dg1", "db1", "WoT", "dfo", "dfod", "dz", "daod", "dao", "dctx")
RBW_ATT_PTRS = ("qkv_a", "P_a", "o_a", "dctx_a", "dP_init", "dqkv_out")
RBW_DIST_PTRS = ("dist", "dsprel_w", "dsprel_b")
assert RBW_PTRS + RBW_ATT_PTRS + RBW_DIST_PTRS == _ptrs(RbwSeg), "include/magic_hip.h: magic_rowbwd_seg's pointer members changed"


_ERR = {-1: "MAGIC_ERR_ARG", -2: "MAGIC_ERR_LAUNCH", -3: "MAGIC_ERR_UNSUPPORTED"}
_lib = None


def source_build_id():
    """the id csrc/build_id.py derives from THIS tree's sources (content hashes; None when the sources are not there)"""
    path = os.path.join(os.path.dirname(_HERE), "csrc", "build_id.py")
    if not os.path.exists(path):
        return None
    import importlib.util
    spec = importlib.util.spec_from_file_location("_magic_build_id", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.build_id()


def library_build_id(lib=None):
    """the id compiled into the loaded libmagic_hip.so (magic_build_id)"""
    lib = lib if lib is not None else load()
    buf = C.create_string_buffer(32)
    if lib.magic_build_id(buf, 32) != 0:
        raise MagicHipError("magic_build_id failed")
    return buf.value.decode()


def check_build_id(lib):
    """a library built from other sources than the tree it sits in is refused (MAGIC_ALLOW_STALE_LIB=1 overrides, for bisecting)"""
    want, got = source_build_id(), library_build_id(lib)
    if want is not None and want != got and not os.environ.get("MAGIC_ALLOW_STALE_LIB"):
        raise MagicHipError(f"{LIB_PATH} was built from other sources (library id {got}, this tree {want}): rebuild with "
                            "`python __graft_entry__.py` (make -C vln-magic_amd/csrc)")


def load():
    """Load the shared library (fails loudly; there is no fallback path)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise MagicHipError(f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                            "(hipcc --offload-arch=gfx950). There is no CPU fallback for the product path.")
    lib = C.CDLL(LIB_PATH)
    for name, args in SIGNATURES.items():
        fn = getattr(lib, name, None)
        if fn is None:
            raise MagicHipError(f"{LIB_PATH} does not export {name}: a stale build -- run `python __graft_entry__.py`")
        fn.argtypes = args
        fn.restype = i32
    check_build_id(lib)
    _lib = lib
    _bind_fast(lib)
    return lib


FAST_PATH = os.environ.get("MAGIC_FASTCALL_PATH") or os.path.join(os.path.dirname(LIB_PATH), "_magic_fastcall.so")     # (env: the sanitizer build, csrc/Makefile `asan`)
_FN = {}          # entry point name -> callable: the generated CPython wrapper when there is one, else the ctypes function


def _fn(name):
    f = _FN.get(name)
    if f is None:
        load()                     # first use: loads the library and fills the table (fails loudly if it is missing)
        f = _FN[name]
    return f


def _bind_fast(lib):
    """`_magic_fastcall` (csrc/gen_fastcall.py -> fastcall.c, built by the same Makefile) converts the plain int / float / pointer
    arguments of a launch in 0.2-0.6 us where ctypes takes 0.5-2.6 us; it calls the SAME loaded libmagic_hip.so.  Entry points with
    struct arguments, and a tree without the extension (MAGIC_NO_FASTCALL=1, or not built), go through ctypes -- same library either way."""
    for name in SIGNATURES:
        _FN[name] = getattr(lib, name)
    if os.environ.get("MAGIC_NO_FASTCALL") or not os.path.exists(FAST_PATH):
        return
    import importlib.util
    spec = importlib.util.spec_from_file_location("_magic_fastcall", FAST_PATH)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.bind(LIB_PATH)
    for name in SIGNATURES:
        f = getattr(mod, name, None)
        if f is not None:
            _FN[name] = f


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def stream():
    """raw handle of torch's current HIP stream on the current device (thread-local, honours torch.cuda.stream contexts).
    `torch.cuda.current_stream()` builds a Stream object and re-resolves the device on every call (~8 us): with ~400 launches
    per eager step that was a third of the host time."""
    if _raw_stream is not None:
        return _raw_stream(torch._C._cuda_getDevice())
    return torch.cuda.current_stream().cuda_stream


def P(t):
    """device pointer of a tensor (None -> NULL)"""
    return None if t is None else t.data_ptr()


PROFILE = {"on": False, "events": []}     # bench.py: per-launch HIP-event timing on the launch stream
PAIRABLE = {"magic_gemm", "magic_attn_fwd", "magic_attn_bwd", "magic_linear_ln", "magic_linear_lnbwd", "magic_ln_bwd", "magic_chain_fwd", "magic_ln_fwd"}
_tls = threading.local()


_DEBUG_SYNC = bool(os.environ.get("MAGIC_DEBUG_SYNC"))     # print + synchronize around every launch (localises a faulting kernel)


def _raw_call(name, args):
    if getattr(_tls, "in_group", False) and name in PAIRABLE:
        rc = _fn(name)(*args)             # recorded by the C side, launched by magic_group_end
        if rc != 0:
            raise MagicHipError(f"{name} failed while recording a group: {_ERR.get(rc, rc)}")
        return
    if _DEBUG_SYNC:
        print("[magic]", name, flush=True)
        rc = _fn(name)(*args)
        torch.cuda.synchronize()
        if rc != 0:
            raise MagicHipError(f"{name} failed: {_ERR.get(rc, rc)}")
        return
    if PROFILE["on"]:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        rc = _fn(name)(*args)
        e1.record()
        PROFILE["events"].append((name, args[1] if name == "magic_gemm" else -1, e0, e1))
        if PROFILE.get("shapes") is not None:       # profiles/micro/nav_kernel_breakdown.py: leading integer arguments (dtype, sizes) per launch
            PROFILE["shapes"].append(tuple(a for a in args[:7] if isinstance(a, int) and abs(a) < (1 << 24)))
    else:
        rc = _fn(name)(*args)
    if rc != 0:
        raise MagicHipError(f"{name} failed: {_ERR.get(rc, rc)}")


class solo:
    """`with L.solo():` -- inside a lockstep segment, launch this thread's groupable calls alone instead of offering them to the partner:
    keeps two segments whose launch sequences differ by a prefix (the panorama encoder's image projection) in phase, so that their layers
    pair kind for kind (QKV with QKV, attention with attention, chain with chain)"""

    def __enter__(self):
        self.prev = getattr(_tls, "solo", False)
        _tls.solo = True
        return self

    def __exit__(self, et, ev, tb):
        _tls.solo = self.prev
        return False


def call(name, *args):
    ls = getattr(_tls, "lockstep", None)
    if ls is not None and name in PAIRABLE and not getattr(_tls, "solo", False):
        return ls.submit(ls.index(), name, args)
    if ls is not None and PROFILE["on"]:
        with ls.cv:            # instrumented pass: keep this launch's event pair free of the partner thread's launches
            return _raw_call(name, args)
    _raw_call(name, args)


class group:
    """`with L.group():` -- the groupable calls (PAIRABLE) issued by THIS thread inside the block are recorded and launched
    together at exit: independent GEMMs of one layout become one grouped launch (<= 8 per block).  The calls must not depend
    on each other, and nothing inside the block may read their outputs.  No-op inside a lockstep segment."""

    def __enter__(self):
        self.on = getattr(_tls, "lockstep", None) is None and not _DEBUG_SYNC
        if self.on:
            if PROFILE["on"]:
                self.ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                self.ev[0].record()
            if load().magic_group_begin() != 0:
                raise MagicHipError("magic_group_begin failed (nested grouping?)")
            _tls.in_group = True
        return self

    def __exit__(self, et, ev, tb):
        if self.on:
            _tls.in_group = False
            rc = load().magic_group_end(stream())
            if PROFILE["on"]:
                self.ev[1].record()
                PROFILE["events"].append(("magic_gemm+group", 0, self.ev[0], self.ev[1]))
            if rc != 0 and et is None:
                raise MagicHipError(f"magic_group_end failed: {_ERR.get(rc, rc)}")
        return False


class Lockstep:
    """Run two independent, same-structured segments (e.g. the global and the local co-attention encoder) on two host
    threads and issue their groupable kernel calls PAIRWISE: when both threads have arrived at a groupable call, the second
    arriver records both through magic_group_begin/…/magic_group_end, which launches ONE kernel serving both problems.
    Non-groupable calls launch immediately.  If one segment finishes first (or raises) the other simply continues alone.

    The two threads ALTERNATE, they never run at the same time: each holds `cv` for as long as it runs (lib.lockstep) and lets go of it only
    while it waits for its partner in `submit`.  The segments are issued into a stream that is being captured, and two threads adding
    nodes to one capturing stream at once can lose one of them from the stream's dependency chain (both read the same last node): the
    capture then ends with hipErrorStreamCaptureUnjoined -- seen once in some hundred captures before the baton."""

    def __init__(self):
        self.cv = threading.Condition()
        self.pending = [None, None]
        self.done = [False, False]
        self.gen = 0
        self.pairs = 0

    def index(self):
        return _tls.idx

    def _meet(self, idx, name, args):
        """the partner is parked at a call: launch both as one group; True when that happened"""
        other = 1 - idx
        if self.pending[other] is None:
            return False
        oname, oargs = self.pending[other]
        first, second = ((oname, oargs), (name, args)) if other == 0 else ((name, args), (oname, oargs))
        lib = load()
        ev = None
        if PROFILE["on"]:
            ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            ev[0].record()
        if lib.magic_group_begin() != 0:
            raise MagicHipError("magic_group_begin failed (nested grouping?)")
        try:
            for n_, a_ in (first, second):
                rc = _fn(n_)(*a_)
                if rc != 0:
                    raise MagicHipError(f"{n_} failed while recording a group: {_ERR.get(rc, rc)}")
        finally:
            rc = lib.magic_group_end(stream())
        if rc != 0:
            raise MagicHipError(f"magic_group_end failed: {_ERR.get(rc, rc)}")
        if ev is not None:
            ev[1].record()
            same = first[0] == second[0]
            PROFILE["events"].append((first[0] + ("+pair" if same else "+" + second[0]), first[1][1] if first[0] == "magic_gemm" else -1, ev[0], ev[1]))
        self.pairs += 1
        self.pending[other] = None
        self.gen += 1
        return True

    def submit(self, idx, name, args):
        other = 1 - idx
        with self.cv:
            if self._meet(idx, name, args):
                self.cv.notify_all()
                return
            if self.done[other]:
                _raw_call(name, args)
                return
            self.pending[idx] = (name, args)
            gen = self.gen
            while self.gen == gen and not self.done[other]:
                self.cv.wait()
            if self.pending[idx] is not None:                    # partner finished without pairing: launch alone
                self.pending[idx] = None
                _raw_call(name, args)

    def finish(self, idx):
        with self.cv:
            self.done[idx] = True
            self.cv.notify_all()


try:
    import greenlet as _greenlet
except ImportError:                       # (the threaded form below needs nothing but the standard library)
    _greenlet = None
LOCKSTEP_FORM = os.environ.get("MAGIC_LOCKSTEP", "greenlets" if _greenlet is not None else "threads")


class LockstepOneThread(Lockstep):
    """The same pairing with NO second thread (round 6): the two segments are two greenlets of the calling thread.  A segment that arrives at a groupable call
    whose twin has not arrived parks the call and switches to the other segment; that one runs until it meets the parked call (both go out as one launch, and
    it carries on), parks a call of its own (and switches back) or ends.  One thread adds nodes to the capturing stream, in an order that is a function of the
    two launch sequences alone -- nothing for a baton to protect.  Segments share the thread's torch state (current stream, grad mode): neither changes it
    around a groupable call."""

    def __init__(self):
        super().__init__()
        self.gl = [None, None]

    def index(self):
        return 0 if _greenlet.getcurrent() is self.gl[0] else 1

    def submit(self, idx, name, args):
        other = 1 - idx
        if self._meet(idx, name, args):
            return
        if self.done[other]:
            _raw_call(name, args)
            return
        self.pending[idx] = (name, args)
        self.gl[other].switch()                               # back here once the partner has met this call, parked one of its own, or ended
        if self.pending[idx] is not None:                     # the partner ended without a twin for it: launch alone
            self.pending[idx] = None
            _raw_call(name, args)


def _lockstep_one_thread(fn_a, fn_b):
    ls = LockstepOneThread()
    box = {}

    def seg(i, fn):
        def run():
            try:
                box[i] = fn()
            finally:
                ls.done[i] = True
        return run
    ls.gl = [_greenlet.greenlet(seg(0, fn_a)), _greenlet.greenlet(seg(1, fn_b))]      # both children of this greenlet: an ended segment returns here
    _tls.lockstep = ls
    try:
        while not (ls.gl[0].dead and ls.gl[1].dead):
            # start / resume the segment that can run: the first, unless it is parked behind a live partner (then the partner is the one mid-flight)
            nxt = 0 if not ls.gl[0].dead and (ls.pending[0] is None or ls.gl[1].dead) else 1
            if ls.gl[nxt].dead:
                nxt = 1 - nxt
            ls.gl[nxt].switch()
    except BaseException:
        for g in ls.gl:                   # unwind the other segment's stack (its `finally` blocks run) before the error leaves
            if g is not None and not g.dead:
                try:
                    g.throw(_greenlet.GreenletExit)
                except BaseException:     # noqa: BLE001
                    pass
        raise
    finally:
        _tls.lockstep = None
    return box[0], box[1]


def lockstep(fn_a, fn_b):
    """returns (fn_a(), fn_b()) with their groupable launches paired (see Lockstep).  Default: both segments on the calling thread (LockstepOneThread);
    MAGIC_LOCKSTEP=threads (or no `greenlet` module): fn_b on a helper thread bound to the caller's device and current stream."""
    if getattr(_tls, "lockstep", None) is not None:              # no nesting: run sequentially inside an outer lockstep
        return fn_a(), fn_b()
    if LOCKSTEP_FORM == "greenlets" and _greenlet is not None:
        return _lockstep_one_thread(fn_a, fn_b)
    ls = Lockstep()
    cur = torch.cuda.current_stream()
    dev = torch.cuda.current_device()
    grad = torch.is_grad_enabled()
    box = {}

    def worker():
        try:
            with ls.cv:                # the baton (see Lockstep): runs only while the caller's thread waits in submit() or has finished
                torch.cuda.set_device(dev)
                _tls.lockstep, _tls.idx = ls, 1
                with torch.cuda.stream(cur), torch.set_grad_enabled(grad):
                    box["b"] = fn_b()
        except BaseException as e:     # noqa: BLE001 - re-raised on the caller's thread
            box["err"] = e
        finally:
            _tls.lockstep = None
            ls.finish(1)

    t = threading.Thread(target=worker, name="magic-lockstep")
    _tls.lockstep, _tls.idx = ls, 0
    try:
        with ls.cv:
            t.start()
            a = fn_a()
    finally:
        _tls.lockstep = None
        ls.finish(0)
        t.join()
    if "err" in box:
        raise box["err"]
    return a, box["b"]


class capture(torch.cuda.graph):
    """`torch.cuda.graph` with Python's cyclic garbage collector OFF for the duration of the capture.  torch collects garbage itself right BEFORE a capture
    begins, but allocations inside a long capture can trigger a collection again, and finalizing an unrelated dead object there (a HIP graph of an earlier
    test / an evicted bucket graph, an event) runs HIP calls the capturing stream does not permit: the destructor throws, the process aborts ("Fatal Python
    error: Aborted ... Garbage-collecting", seen once in round 6 in a full GPU suite run, inside StreamStep's capture).  The garbage is collected after the capture ends."""

    def __enter__(self):
        import gc
        self._gc_was = gc.isenabled()
        r = super().__enter__()
        gc.disable()
        return r

    def __exit__(self, *exc):
        import gc
        try:
            return super().__exit__(*exc)
        finally:
            if self._gc_was:
                gc.enable()


def set_f32_mfma(mode):
    """contraction arithmetic of the fp32 storage mode: 'exact' (v_mfma_f32_16x16x4_f32) or 'bf16x3' (split-bf16, three bf16 MFMAs per
    product, ~2^-17 relative error).  Process-wide; returns the previous mode."""
    lib = load()
    prev = "bf16x3" if lib.magic_get_f32_mfma() else "exact"
    want = {"exact": 0, "bf16x3": 1}[mode]
    torch.cuda.synchronize()
    rc = lib.magic_set_f32_mfma(want)
    if rc != 0:
        raise MagicHipError(f"magic_set_f32_mfma failed: {_ERR.get(rc, rc)}")
    return prev


HALF = (torch.bfloat16, torch.float16)     # the two 16-bit storage types: every MFMA kernel exists for both (csrc/common.hpp H16<>)


def dt(dtype):
    if dtype == torch.float32:
        return 0
    if dtype == torch.bfloat16:
        return 1
    if dtype == torch.float16:
        return 2
    raise MagicHipError(f"unsupported compute dtype {dtype}")
