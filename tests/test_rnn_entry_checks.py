"""What the ten entry points of the LSTM and GRU recurrences check before they launch anything, entry by entry: the
required and the optional pointers, the workspace's alignment and size, the sizes no plan covers, nblk = 0 and
nblk > INT32_MAX.  All ten run the same sequence (pointers and ranges, plan, workspace, nblk == 0, then the launch); this
table is each one's own contract with it.

Every check under test returns before any HIP call, so no GPU is needed and the pointers are fakes (4096: non-NULL and
16-byte aligned).  No case here may let a call with fake pointers get past the workspace check with nblk > 0: `Entry`
refuses to make a call whose size has a plan unless nblk is 0 or workspace_bytes is below what that launch needs.

What a launch needs is not always what the workspace query answers: the query is one bound per (cell, nbatch, size) for
the forward and the backward (the LSTM's is the backward's at 16 units per workgroup, above every plan's; the GRU's at
size 256 is the backward's, four times the forward's).  A call one byte under the QUERY can therefore pass the check and
launch, so the byte that is asserted to be missed is the last one of the launch's own need: the plan's forward or
backward granule bytes (tk_lab_lstm_geometry; for the GRU the forward-only query and the training query, which are
exactly the two).  Where need and query agree -- every entry of the forward-only library, the GRU's backward, the GRU
at sizes <= 128 -- that is `query - 1`."""
import ctypes
import functools

import pytest

from taiyaki_amd import _lib

BAD_ARG, UNSUPPORTED, WORKSPACE = (_lib.DEFINES["TK_ERR_" + k] for k in ("BAD_ARG", "UNSUPPORTED", "WORKSPACE"))
OK = 0
SCALARS = ("nblk", "nbatch", "size", "reverse", "cu_count", "workspace_bytes", "stream")
TAIL = "nblk nbatch size reverse cu_count"
END = "workspace workspace_bytes status stream"

# entry -> (library, workspace query, arguments in the header's order, the pointers that may be NULL)
ENTRIES = {
    "tk_lstm_forward_dev": ("lib", "lstm", "gx w_hh %s y gates cell %s" % (TAIL, END), ()),
    "tk_lstm_backward_dev": ("lib", "lstm", "w_hh gates cell dy %s dgates %s" % (TAIL, END), ()),
    "tk_gru_forward_dev": ("lib", "gru", "gx w_hh b_hh %s y gates q %s" % (TAIL, END), ("gates", "q")),
    "tk_gru_backward_dev": ("lib", "gru", "w_hh y gates q dy %s dgates dq %s" % (TAIL, END), ()),
    "tk_lstm_forward_varlen_dev": ("varlen_lib", "lstm", "gx w_hh lengths %s y %s" % (TAIL, END), ("lengths",)),
    "tk_gru_forward_varlen_dev": ("varlen_lib", "gru", "gx w_hh b_hh lengths %s y %s" % (TAIL, END), ("lengths",)),
    "tk_lstm_forward_varlen_save_dev": ("varlen_train_lib", "lstm", "gx w_hh lengths %s y gates cell %s" % (TAIL, END),
                                        ("lengths",)),
    "tk_lstm_backward_varlen_dev": ("varlen_train_lib", "lstm", "w_hh gates cell dy lengths %s dgates %s" % (TAIL, END),
                                    ("lengths",)),
    "tk_gru_forward_varlen_save_dev": ("varlen_train_lib", "gru", "gx w_hh b_hh lengths %s y gates q %s" % (TAIL, END),
                                       ("lengths",)),
    "tk_gru_backward_varlen_dev": ("varlen_train_lib", "gru",
                                   "w_hh y gates q dy lengths %s dgates dq %s" % (TAIL, END), ("lengths",)),
}
SIZES = {"lstm": [(4, 64, 256), (5, 256, 256)], "gru": [(4, 64, 256), (5, 256, 256), (6, 96, 256)]}
CASES = [(name, shape) for name, (_, cell, _, _) in ENTRIES.items() for shape in SIZES[cell]]


def _kind(cell):
    return 0 if cell == "lstm" else 1


def _query(libname, cell, nbatch, size, cu_count):
    L = getattr(_lib, libname)()
    if libname == "lib":
        return getattr(L, "tk_%s_workspace_bytes" % cell)(nbatch, size, cu_count)
    q = L.tk_rnn_varlen_workspace_bytes if libname == "varlen_lib" else L.tk_rnn_varlen_train_workspace_bytes
    return q(_kind(cell), nbatch, size, cu_count)


@functools.lru_cache(maxsize=None)
def _lstm_granule_bytes(nbatch, size, cu_count):
    """(forward, backward) granule bytes of the launch plan, from the library's own plan (the lab build, nothing forced)"""
    L = _lib.use_lab(True)
    try:
        out = (ctypes.c_size_t * 8)()
        assert L.tk_lab_lstm_geometry(nbatch, size, cu_count, out)
        return int(out[6]), int(out[7])
    finally:
        _lib.use_lab(False)


class Entry:
    def __init__(self, name, shape):
        libname, self.cell, names, self.optional = ENTRIES[name]
        self.names = names.split()
        self.nbatch, self.size, self.cu_count = shape
        backward = "backward" in name
        if self.cell == "lstm":
            self.need = _lstm_granule_bytes(*shape)[backward]
        else:
            self.need = _query("varlen_train_lib" if backward else "varlen_lib", "gru", *shape)
        self.fn = getattr(getattr(_lib, libname)(), name)
        self.query = _query(libname, self.cell, *shape)
        self.pointers = [n for n in self.names if n not in SCALARS]

    def __call__(self, **over):
        """The call with fake pointers everywhere, nblk = 4 and workspace_bytes = 0; `over` replaces arguments by name."""
        args = dict(nblk=4, nbatch=self.nbatch, size=self.size, reverse=0, cu_count=self.cu_count, workspace_bytes=0,
                    stream=None)
        args.update({n: ctypes.c_void_p(4096) for n in self.pointers})
        assert set(over) <= set(args), over
        args.update(over)
        assert args["nblk"] == 0 or args["workspace_bytes"] < self.need or args["size"] == 48, "this call could launch"
        return self.fn(*[args[n] for n in self.names])


def test_the_table_is_the_bindings():
    sigs = dict(_lib.SIGNATURES)
    sigs.update(_lib.VARLEN_SIGNATURES)
    sigs.update(_lib.VARLEN_TRAIN_SIGNATURES)
    for name, (_, _, names, optional) in ENTRIES.items():
        names = names.split()
        restype, argtypes = sigs[name][:2]
        assert restype is ctypes.c_int and len(argtypes) == len(names), name
        for n, t in zip(names, argtypes):
            want = ctypes.c_void_p if n not in SCALARS or n == "stream" else \
                ctypes.c_int if n in ("reverse", "cu_count") else ctypes.c_size_t
            assert t is want, (name, n)
        assert set(optional) <= set(names)


@pytest.mark.parametrize("name,shape", CASES, ids=["%s-%d-%d-%d" % ((n,) + s) for n, s in CASES])
def test_entry_checks(name, shape):
    e = Entry(name, shape)
    assert 0 < e.need <= e.query and e.need % 16 == 0
    assert "workspace" in e.pointers and "status" in e.pointers and not set(e.optional) & {"workspace", "status"}
    # required pointers, one at a time; the workspace's alignment.  (The pointer check is the first: it answers
    # whatever workspace_bytes says, so these calls pass 0 and could not launch if the check were gone.)
    for p in e.pointers:
        if p not in e.optional:
            assert e(**{p: None}) == BAD_ARG, p
    assert e(workspace=ctypes.c_void_p(4100)) == BAD_ARG
    # optional pointers: the call passes the pointer check and stops at the workspace's size
    assert e() == WORKSPACE
    for p in e.optional:
        assert e(**{p: None}) == WORKSPACE, p
    assert e(**{p: None for p in e.optional}) == WORKSPACE
    # a size with no plan, whatever the workspace
    assert e(size=48, workspace_bytes=1 << 40) == UNSUPPORTED
    assert e(size=48) == UNSUPPORTED
    # the last byte of the launch's need (the module docstring: `query - 1` wherever the query is that need)
    assert e(workspace_bytes=e.need - 1) == WORKSPACE
    if "varlen_dev" in name and "backward" not in name or (e.cell == "gru" and ("backward" in name or e.size <= 128)):
        assert e.need == e.query
    if (e.cell, e.size) == ("gru", 96):
        assert e.query == 16 and e(workspace_bytes=15) == WORKSPACE
    # nblk = 0: nothing to do, and nothing is touched (the return sits in front of the workspace's zeroing); the
    # workspace is still checked
    assert e(nblk=0, workspace_bytes=e.query) == OK
    assert e(nblk=0, workspace_bytes=e.need) == OK
    assert e(nblk=0, workspace_bytes=e.need - 1) == WORKSPACE
    # nblk beyond int32 (the range check sits with the pointers', in front of the workspace's)
    assert e(nblk=2 ** 31) == BAD_ARG
    assert e(nblk=2 ** 31 - 1) == WORKSPACE
