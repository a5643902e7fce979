"""ctypes binding of the C ABI in include/taiyaki_amd_flipflop.h.

PyTorch is plumbing here (device memory, streams); every hot-path computation
is a HIP kernel behind the C ABI.  There is NO CPU / eager fallback: if the
shared library is missing or a tensor is not on an AMD GPU the operators raise.
"""
import ctypes
import os
import re
import subprocess

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
LIBNAME = "libtaiyaki_amd_flipflop.so"
LIBPATH = os.environ.get("TAIYAKI_AMD_LIB") or os.path.join(CSRC, LIBNAME)   # (override: lab builds)
# The LAB build of the same sources (-DTK_LAB): the only one that reads the dispatch's environment switches
# (TK_CRF_MODE, TK_CRF_BK, TK_LOGZ_CH, TK_CRF_NO_FALLBACK ...) and exports tk_lab_*.  tests/ and tools/ switch
# to it with `use_lab()` when they flip one; the operators never load it by themselves.
LAB_LIBNAME = "libtaiyaki_amd_flipflop_lab.so"
LAB_LIBPATH = os.environ.get("TAIYAKI_AMD_LAB_LIB") or os.path.join(CSRC, LAB_LIBNAME)    # (override: A/B builds under tools/lab/)

HEADER = os.path.join(os.path.dirname(_HERE), "include", "taiyaki_amd_flipflop.h")
RCCL_LIBNAME = "libtaiyaki_amd_rccl.so"     # csrc/rccl_api.cpp: the header's multi-GPU section, a library of its own
BASECALL_HEADER = os.path.join(os.path.dirname(_HERE), "include", "taiyaki_amd_basecall.h")
BASECALL_LIBNAME = "libtaiyaki_amd_basecall.so"     # csrc/basecall_kernels.hip: the basecaller's glue, header and library of its own

WGRAD_HEADER = os.path.join(os.path.dirname(_HERE), "include", "taiyaki_amd_lstm_wgrad.h")
WGRAD_LIBNAME = "libtaiyaki_amd_lstm_wgrad.so"      # csrc/lstm_wgrad.hip: the LSTM's parameter gradients, header and library of its own
WGRAD_LAB_LIBNAME = "libtaiyaki_amd_lstm_wgrad_lab.so"      # ... and its lab build (tk_lab_lstm_wgrad_*)
GRU_WGRAD_HEADER = os.path.join(os.path.dirname(_HERE), "include", "taiyaki_amd_gru_wgrad.h")
GRU_WGRAD_LIBNAME = "libtaiyaki_amd_gru_wgrad.so"   # csrc/gru_wgrad.hip: the GRU's parameter gradients, header and library of its own
GRU_WGRAD_LAB_LIBNAME = "libtaiyaki_amd_gru_wgrad_lab.so"   # ... and its lab build (tk_lab_gru_wgrad_*)
RNN_PROJ_HEADER = os.path.join(os.path.dirname(_HERE), "include", "taiyaki_amd_rnn_proj.h")
RNN_PROJ_LIBNAME = "libtaiyaki_amd_rnn_proj.so"     # csrc/rnn_proj.hip: the recurrent layers' projection GEMMs, header and library of its own
RNN_PROJ_LAB_LIBNAME = "libtaiyaki_amd_rnn_proj_lab.so"     # ... and its lab build (tk_lab_rnn_proj_plan)
CONV_STRIDED_HEADER = os.path.join(os.path.dirname(_HERE), "include", "taiyaki_amd_conv_strided.h")
CONV_STRIDED_LIBNAME = "libtaiyaki_amd_conv_strided.so"     # csrc/conv_strided.hip: the 16 -> Cout stride-5 convolution, header and library of its own
CONV_STRIDED_LAB_LIBNAME = "libtaiyaki_amd_conv_strided_lab.so"     # ... and its lab build (tk_lab_conv_strided_*)
SQUIGGLE_NET_HEADER = os.path.join(os.path.dirname(_HERE), "include", "taiyaki_amd_squiggle_net.h")
SQUIGGLE_NET_LIBNAME = "libtaiyaki_amd_squiggle_net.so"     # csrc/squiggle_net.hip: the squiggle predictor network in one launch per pass, header and library of its own
SQUIGGLE_NET_LAB_LIBNAME = "libtaiyaki_amd_squiggle_net_lab.so"     # ... and its lab build (tk_lab_squiggle_net_plan)
LSTM_LOCAL_HEADER = os.path.join(os.path.dirname(_HERE), "include", "taiyaki_amd_lstm_local.h")
LSTM_LOCAL_LIBNAME = "libtaiyaki_amd_lstm_local.so"     # csrc/lstm_local.hip: the LSTM recurrence at size 96, one workgroup per column set, header and library of its own
LSTM_LOCAL_LAB_LIBNAME = "libtaiyaki_amd_lstm_local_lab.so"     # ... and its lab build (tk_lab_lstm_local_cols)
LSTM_LARGE_HEADER = os.path.join(os.path.dirname(_HERE), "include", "taiyaki_amd_lstm_large.h")
LSTM_LARGE_LIBNAME = "libtaiyaki_amd_lstm_large.so"     # csrc/lstm_kernels.hip built -DTK_LSTM_LARGE: the LSTM recurrence at size 512, header and library of its own
LSTM_LARGE_LAB_LIBNAME = "libtaiyaki_amd_lstm_large_lab.so"     # ... and its lab build (tk_lab_lstm_large_cols, tk_lab_lstm_large_geometry)
ALIGN_HEADER = os.path.join(os.path.dirname(_HERE), "include", "taiyaki_amd_align.h")
ALIGN_LIBNAME = "libtaiyaki_amd_align.so"       # csrc/align_kernels.hip: edit-distance alignment of batches of pairs, header and library of its own
CONV_SIGNAL_HEADER = os.path.join(os.path.dirname(_HERE), "include", "taiyaki_amd_conv_signal.h")
CONV_SIGNAL_LIBNAME = "libtaiyaki_amd_conv_signal.so"       # csrc/conv_signal.hip: the 1 -> Cout convolution on the raw signal (tanh), header and library of its own
OUT_LAYER_HEADER = os.path.join(os.path.dirname(_HERE), "include", "taiyaki_amd_out_layer.h")
OUT_LAYER_LIBNAME = "libtaiyaki_amd_out_layer.so"       # csrc/out_layer.hip: the models' output layer (plain and cat-mod), header and library of its own
OUT_LAYER_LAB_LIBNAME = "libtaiyaki_amd_out_layer_lab.so"       # ... and its lab build (tk_lab_out_layer_plan)
CONV_WINDOW_HEADER = os.path.join(os.path.dirname(_HERE), "include", "taiyaki_amd_conv_window.h")
CONV_WINDOW_LIBNAME = "libtaiyaki_amd_conv_window.so"       # csrc/conv_strided.hip built -DTK_CONV_WINDOW: the 16 -> Cout convolution at the fast and RNA shapes, header and library of its own
CONV_WINDOW_LAB_LIBNAME = "libtaiyaki_amd_conv_window_lab.so"       # ... and its lab build (tk_lab_conv_window_*)
CHUNKS_SEQLEN_HEADER = os.path.join(os.path.dirname(_HERE), "include", "taiyaki_amd_chunks_seqlen.h")
CHUNKS_SEQLEN_LIBNAME = "libtaiyaki_amd_chunks_seqlen.so"       # csrc/chunk_seqlen.hip: chunks of a fixed number of bases (the squiggle trainer's batches), header and library of its own
OPTIM_HEADER = os.path.join(os.path.dirname(_HERE), "include", "taiyaki_amd_optim.h")
OPTIM_LIBNAME = "libtaiyaki_amd_optim.so"       # csrc/optim.hip: the optimiser step (scale, maxima, clamp, norm cap, AdamW, zero fill), header and library of its own

VARLEN_HEADER = os.path.join(os.path.dirname(_HERE), "include", "taiyaki_amd_rnn_varlen.h")
VARLEN_LIBNAME = "libtaiyaki_amd_rnn_varlen.so"     # csrc/lstm_kernels.hip, gru_kernels.hip built -DTK_RNN_VARLEN: header and library of its own

VARLEN_TRAIN_HEADER = os.path.join(os.path.dirname(_HERE), "include", "taiyaki_amd_rnn_varlen_train.h")
VARLEN_TRAIN_LIBNAME = "libtaiyaki_amd_rnn_varlen_train.so"     # the same two sources built -DTK_RNN_VARLEN_TRAIN: the training pair with per-column lengths
WIDE_HEADER = os.path.join(os.path.dirname(_HERE), "include", "taiyaki_amd_rnn_wide.h")
WIDE_LIBNAME = "libtaiyaki_amd_rnn_wide.so"     # the same two sources built -DTK_RNN_WIDE: every batch width, as slabs of columns
DECODE_VARLEN_HEADER = os.path.join(os.path.dirname(_HERE), "include", "taiyaki_amd_decode_varlen.h")
DECODE_VARLEN_LIBNAME = "libtaiyaki_amd_decode_varlen.so"   # csrc/decode_varlen.hip: the decode operators with per-column lengths, header and library of its own

LOSS_VARLEN_HEADER = os.path.join(os.path.dirname(_HERE), "include", "taiyaki_amd_loss_varlen.h")
LOSS_VARLEN_LIBNAME = "libtaiyaki_amd_loss_varlen.so"       # csrc/crf_band.hip, crf_kernels.hip built -DTK_LOSS_VARLEN: the loss with a time length per column

_vp = ctypes.c_void_p
_SCALARS = {"size_t": ctypes.c_size_t, "int": ctypes.c_int, "float": ctypes.c_float}


def _ctype(decl, where, named=True):
    """The ctypes type of one C declarator (`const float *x`, `size_t n`), or of a result type (named=False).
    Anything outside the map raises: the binding never guesses."""
    words = decl.replace("*", " * ").split()
    base, stars = [w for w in words if w not in ("*", "const")], words.count("*")
    if len(base) == 1 + named:
        if stars == 1:
            return ctypes.c_char_p if base[0] == "char" and "const" in words else _vp
        if stars == 2 and base[0] == "void":
            return ctypes.POINTER(_vp)
        if stars == 0 and base[0] in _SCALARS:
            return _SCALARS[base[0]]
        if stars == 0 and base[0] == "void" and not named:
            return None
    raise TypeError("%s: no ctypes type for `%s`" % (where, " ".join(words)))


def _blank_comments(text):      # ... and preprocessor lines, with spaces: offsets into the text stay what they were
    return re.sub(r"/\*.*?\*/|//[^\n]*|(?m:^[ \t]*#[^\n]*)", lambda m: " " * len(m.group()), text, flags=re.S)


def parse_prototypes(text):
    """C prototypes (comments blanked, one declarator per parameter) -> {name: (restype, argtypes, offset in text)}"""
    out = {}
    for m in re.finditer(r"(\w[\w\s*]*?)\b(\w+)\s*\(([^()]*)\)\s*;", text):
        res, name, params = m.groups()
        params = [] if params.strip() in ("", "void") else params.split(",")
        out[name] = (_ctype(res, name, named=False), [_ctype(p, name) for p in params], m.start(2))
    return out


def _read_header():
    raw = open(HEADER).read()
    text = _blank_comments(raw)
    protos, multi_gpu = parse_prototypes(text), raw.index("Multi-GPU:")
    sigs = {n: (r, a) for n, (r, a, at) in protos.items() if at < multi_gpu}
    rccl = {n: (r, a) for n, (r, a, at) in protos.items() if at > multi_gpu}
    fields = re.search(r"typedef struct tk_seq_labels \{(.*?)\}", text, re.S).group(1).split(";")[:-1]
    fields = [(f.replace("*", " ").split()[-1], _ctype(f, "tk_seq_labels")) for f in fields]
    defines = {k: int(v.rstrip("u"), 0) for k, v in re.findall(r"(?m)^#define (TK_\w+) (\w+)", raw) if v[0].isdigit()}
    return sigs, rccl, fields, defines


# symbol -> (restype, argtypes), read from include/taiyaki_amd_flipflop.h; RCCL_SIGNATURES: its multi-GPU section (the all-reduce
# straight on RCCL for hosts without torch.distributed; the Python trainers use ProcessGroupNCCL and never load that library)
SIGNATURES, RCCL_SIGNATURES, _seq_label_fields, DEFINES = _read_header()
# the tk_lab_* hooks of the lab build: the extern "C" block that csrc/dispatch.h declares under TK_LAB
LAB_SIGNATURES = {n: (r, a) for n, (r, a, _) in parse_prototypes(_blank_comments(re.search(
    r'#ifdef TK_LAB\nextern "C" \{\n(.*?)\n\}\n#endif', open(os.path.join(CSRC, "dispatch.h")).read(), re.S).group(1))).items()}


def _read_basecall_header():
    raw = open(BASECALL_HEADER).read()
    sigs = {n: (r, a) for n, (r, a, _) in parse_prototypes(_blank_comments(raw)).items()}
    return sigs, {k: int(v.rstrip("u"), 0) for k, v in re.findall(r"(?m)^#define (TK_\w+) (\w+)", raw) if v[0].isdigit()}


# the fourth table: include/taiyaki_amd_basecall.h (libtaiyaki_amd_basecall.so), and its status bits
BASECALL_SIGNATURES, BASECALL_DEFINES = _read_basecall_header()


def _read_wgrad_header(header=WGRAD_HEADER):
    sigs = {n: (r, a) for n, (r, a, _) in parse_prototypes(_blank_comments(open(header).read())).items()}
    return ({n: v for n, v in sigs.items() if not n.startswith("tk_lab_")},
            {n: v for n, v in sigs.items() if n.startswith("tk_lab_")})


# the fifth: include/taiyaki_amd_lstm_wgrad.h (libtaiyaki_amd_lstm_wgrad.so), and the hooks its lab build adds
WGRAD_SIGNATURES, WGRAD_LAB_SIGNATURES = _read_wgrad_header()
# the ninth: include/taiyaki_amd_gru_wgrad.h (libtaiyaki_amd_gru_wgrad.so), and the hooks its lab build adds
GRU_WGRAD_SIGNATURES, GRU_WGRAD_LAB_SIGNATURES = _read_wgrad_header(GRU_WGRAD_HEADER)
# the tenth: include/taiyaki_amd_rnn_proj.h (libtaiyaki_amd_rnn_proj.so), and the hook its lab build adds
RNN_PROJ_SIGNATURES, RNN_PROJ_LAB_SIGNATURES = _read_wgrad_header(RNN_PROJ_HEADER)
# the eleventh: include/taiyaki_amd_conv_strided.h (libtaiyaki_amd_conv_strided.so), and the hooks its lab build adds
CONV_STRIDED_SIGNATURES, CONV_STRIDED_LAB_SIGNATURES = _read_wgrad_header(CONV_STRIDED_HEADER)
# the thirteenth: include/taiyaki_amd_squiggle_net.h (libtaiyaki_amd_squiggle_net.so), and the hook its lab build adds
SQUIGGLE_NET_SIGNATURES, SQUIGGLE_NET_LAB_SIGNATURES = _read_wgrad_header(SQUIGGLE_NET_HEADER)
# the fifteenth: include/taiyaki_amd_lstm_local.h (libtaiyaki_amd_lstm_local.so), and the hook its lab build adds
LSTM_LOCAL_SIGNATURES, LSTM_LOCAL_LAB_SIGNATURES = _read_wgrad_header(LSTM_LOCAL_HEADER)


def _read_varlen_header():
    raw = open(VARLEN_HEADER).read()
    sigs = {n: (r, a) for n, (r, a, _) in parse_prototypes(_blank_comments(raw)).items()}
    return sigs, {k: int(v, 0) for k, v in re.findall(r"(?m)^#define (TK_RNN_KIND_\w+) (\d+)", raw)}


# the sixth: include/taiyaki_amd_rnn_varlen.h (libtaiyaki_amd_rnn_varlen.so), and its TK_RNN_KIND_* values
VARLEN_SIGNATURES, VARLEN_DEFINES = _read_varlen_header()


# the seventh: include/taiyaki_amd_decode_varlen.h (libtaiyaki_amd_decode_varlen.so)
DECODE_VARLEN_SIGNATURES = {n: (r, a) for n, (r, a, _) in
                            parse_prototypes(_blank_comments(open(DECODE_VARLEN_HEADER).read())).items()}


# the eighth: include/taiyaki_amd_rnn_varlen_train.h (libtaiyaki_amd_rnn_varlen_train.so)
VARLEN_TRAIN_SIGNATURES = {n: (r, a) for n, (r, a, _) in
                           parse_prototypes(_blank_comments(open(VARLEN_TRAIN_HEADER).read())).items()}


# the twelfth: include/taiyaki_amd_rnn_wide.h (libtaiyaki_amd_rnn_wide.so)
WIDE_SIGNATURES = {n: (r, a) for n, (r, a, _) in parse_prototypes(_blank_comments(open(WIDE_HEADER).read())).items()}


# the fourteenth: include/taiyaki_amd_loss_varlen.h (libtaiyaki_amd_loss_varlen.so)
LOSS_VARLEN_SIGNATURES = {n: (r, a) for n, (r, a, _) in
                          parse_prototypes(_blank_comments(open(LOSS_VARLEN_HEADER).read())).items()}


def _read_align_header():
    raw = open(ALIGN_HEADER).read()
    sigs = {n: (r, a) for n, (r, a, _) in parse_prototypes(_blank_comments(raw)).items()}
    return sigs, {k: int(v) for k, v in re.findall(r"(?m)^#define (TK_ALIGN_\w+) (\d+)", raw)}


# the sixteenth: include/taiyaki_amd_align.h (libtaiyaki_amd_align.so), and its limits
ALIGN_SIGNATURES, ALIGN_DEFINES = _read_align_header()


# the seventeenth: include/taiyaki_amd_conv_signal.h (libtaiyaki_amd_conv_signal.so)
CONV_SIGNAL_SIGNATURES = {n: (r, a) for n, (r, a, _) in
                          parse_prototypes(_blank_comments(open(CONV_SIGNAL_HEADER).read())).items()}


# the eighteenth: include/taiyaki_amd_out_layer.h (libtaiyaki_amd_out_layer.so), and the hook its lab build adds
OUT_LAYER_SIGNATURES, OUT_LAYER_LAB_SIGNATURES = _read_wgrad_header(OUT_LAYER_HEADER)
# the nineteenth: include/taiyaki_amd_conv_window.h (libtaiyaki_amd_conv_window.so), and the hooks its lab build adds
CONV_WINDOW_SIGNATURES, CONV_WINDOW_LAB_SIGNATURES = _read_wgrad_header(CONV_WINDOW_HEADER)
# the twentieth: include/taiyaki_amd_chunks_seqlen.h (libtaiyaki_amd_chunks_seqlen.so)
CHUNKS_SEQLEN_SIGNATURES = {n: (r, a) for n, (r, a, _) in
                            parse_prototypes(_blank_comments(open(CHUNKS_SEQLEN_HEADER).read())).items()}


def _read_optim_header():
    raw = open(OPTIM_HEADER).read()
    sigs = {n: (r, a) for n, (r, a, _) in parse_prototypes(_blank_comments(raw)).items()}
    return sigs, {k: int(v) for k, v in re.findall(r"(?m)^#define (TK_OPTIM_\w+) (\d+)", raw)}


# the twenty-first: include/taiyaki_amd_optim.h (libtaiyaki_amd_optim.so), its tile length and the words of its hyper block
OPTIM_SIGNATURES, OPTIM_DEFINES = _read_optim_header()
# the twenty-second: include/taiyaki_amd_lstm_large.h (libtaiyaki_amd_lstm_large.so), and the hooks its lab build adds
LSTM_LARGE_SIGNATURES, LSTM_LARGE_LAB_SIGNATURES = _read_wgrad_header(LSTM_LARGE_HEADER)


class SeqLabels(ctypes.Structure):
    """include/taiyaki_amd_flipflop.h: tk_seq_labels (what tk_flipflop_build_indices_dev takes, for the entry points
    that build their indices inside their first launch)."""
    _fields_ = _seq_label_fields


ERRORS = {DEFINES["TK_ERR_" + name]: text for name, text in dict(
    BAD_ARG="bad argument (NULL / shape / 16-byte alignment)", WORKSPACE="workspace too small", LAUNCH="HIP launch failure",
    UNSUPPORTED="unsupported nbase / ntrans / sequence length for this build").items()}

_lib = None
_handles = {}


def build(force=False):
    """Compile the gfx950 shared libraries in-tree (hipcc cross-compiles without a GPU)."""
    if force:
        subprocess.run(["make", "-C", CSRC, "clean"], check=True, stdout=subprocess.DEVNULL)
    subprocess.run(["make", "-C", CSRC, "-j%d" % min(8, os.cpu_count() or 4)], check=True,
                   stdout=subprocess.DEVNULL)
    return LIBPATH


def _load(path, signatures):
    handle = _handles.get(path)
    if handle is None:
        if not os.path.exists(path):
            raise RuntimeError(
                "%s is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(there is no CPU fallback for the flip-flop operators)" % path)
        handle = ctypes.CDLL(path)
        for name, (res, args) in signatures.items():
            fn = getattr(handle, name)      # AttributeError if the symbol is not exported
            fn.restype = res
            fn.argtypes = args
        _handles[path] = handle
    return handle


def lib():
    global _lib
    if _lib is None:
        _lib = _load(LIBPATH, SIGNATURES)
    return _lib


def use_lab(flag=True):
    """Route the operators of THIS process through the lab build (flag) or back through the release
    library.  Returns the handle now in use.  Lab switches (environment variables read per launch,
    tk_lab_*) only exist there; the two libraries keep separate side queues and caches."""
    global _lib
    _lib = _load(LAB_LIBPATH, dict(SIGNATURES, **LAB_SIGNATURES)) if flag else _load(LIBPATH, SIGNATURES)
    return _lib


def is_lab():
    return _lib is not None and _lib is _handles.get(LAB_LIBPATH)


_rccl = None


def rccl_lib():
    """The RCCL C-ABI library (loads librccl: only for hosts that want the collective without
    torch.distributed)."""
    global _rccl
    if _rccl is None:
        _rccl = _load(os.path.join(CSRC, RCCL_LIBNAME), RCCL_SIGNATURES)
    return _rccl


_basecall = None


def basecall_lib():
    """The basecaller's glue kernels (include/taiyaki_amd_basecall.h).  No fallback: a missing library raises."""
    global _basecall
    if _basecall is None:
        _basecall = _load(os.path.join(CSRC, BASECALL_LIBNAME), BASECALL_SIGNATURES)
    return _basecall


def wgrad_lib():
    """The LSTM's parameter gradients (include/taiyaki_amd_lstm_wgrad.h): the lab build of that library while the
    process runs on the lab build (`use_lab`), the release one otherwise.  No fallback: a missing library raises."""
    if is_lab():
        return _load(os.path.join(CSRC, WGRAD_LAB_LIBNAME), dict(WGRAD_SIGNATURES, **WGRAD_LAB_SIGNATURES))
    return _load(os.path.join(CSRC, WGRAD_LIBNAME), WGRAD_SIGNATURES)


def gru_wgrad_lib():
    """The GRU's parameter gradients (include/taiyaki_amd_gru_wgrad.h): the lab build of that library while the
    process runs on the lab build (`use_lab`), the release one otherwise.  No fallback: a missing library raises."""
    if is_lab():
        return _load(os.path.join(CSRC, GRU_WGRAD_LAB_LIBNAME),
                     dict(GRU_WGRAD_SIGNATURES, **GRU_WGRAD_LAB_SIGNATURES))
    return _load(os.path.join(CSRC, GRU_WGRAD_LIBNAME), GRU_WGRAD_SIGNATURES)


def rnn_proj_lib():
    """The recurrent layers' projection GEMMs (include/taiyaki_amd_rnn_proj.h): the lab build of that library while the
    process runs on the lab build (`use_lab`), the release one otherwise.  No fallback: a missing library raises."""
    if is_lab():
        return _load(os.path.join(CSRC, RNN_PROJ_LAB_LIBNAME),
                     dict(RNN_PROJ_SIGNATURES, **RNN_PROJ_LAB_SIGNATURES))
    return _load(os.path.join(CSRC, RNN_PROJ_LIBNAME), RNN_PROJ_SIGNATURES)


def conv_strided_lib():
    """The 16 -> Cout, window 19, stride 5 convolution (include/taiyaki_amd_conv_strided.h): the lab build of that
    library while the process runs on the lab build (`use_lab`), the release one otherwise.  No fallback: a missing
    library raises."""
    if is_lab():
        return _load(os.path.join(CSRC, CONV_STRIDED_LAB_LIBNAME),
                     dict(CONV_STRIDED_SIGNATURES, **CONV_STRIDED_LAB_SIGNATURES))
    return _load(os.path.join(CSRC, CONV_STRIDED_LIBNAME), CONV_STRIDED_SIGNATURES)


def squiggle_net_lib():
    """The squiggle predictor network (include/taiyaki_amd_squiggle_net.h): the lab build of that library while the
    process runs on the lab build (`use_lab`), the release one otherwise.  No fallback: a missing library raises."""
    if is_lab():
        return _load(os.path.join(CSRC, SQUIGGLE_NET_LAB_LIBNAME),
                     dict(SQUIGGLE_NET_SIGNATURES, **SQUIGGLE_NET_LAB_SIGNATURES))
    return _load(os.path.join(CSRC, SQUIGGLE_NET_LIBNAME), SQUIGGLE_NET_SIGNATURES)


def lstm_local_lib():
    """The LSTM recurrence at a size one workgroup holds (include/taiyaki_amd_lstm_local.h): the lab build of that
    library while the process runs on the lab build (`use_lab`), the release one otherwise.  No fallback: a missing
    library raises."""
    if is_lab():
        return _load(os.path.join(CSRC, LSTM_LOCAL_LAB_LIBNAME),
                     dict(LSTM_LOCAL_SIGNATURES, **LSTM_LOCAL_LAB_SIGNATURES))
    return _load(os.path.join(CSRC, LSTM_LOCAL_LIBNAME), LSTM_LOCAL_SIGNATURES)


def lstm_large_lib():
    """The LSTM recurrence at hidden size 512 (include/taiyaki_amd_lstm_large.h): the lab build of that library while
    the process runs on the lab build (`use_lab`), the release one otherwise.  No fallback: a missing library raises."""
    if is_lab():
        return _load(os.path.join(CSRC, LSTM_LARGE_LAB_LIBNAME),
                     dict(LSTM_LARGE_SIGNATURES, **LSTM_LARGE_LAB_SIGNATURES))
    return _load(os.path.join(CSRC, LSTM_LARGE_LIBNAME), LSTM_LARGE_SIGNATURES)


def align_lib():
    """The alignment kernels behind taiyaki_amd.accuracy (include/taiyaki_amd_align.h).  No fallback: a missing library
    raises."""
    return _load(os.path.join(CSRC, ALIGN_LIBNAME), ALIGN_SIGNATURES)


def conv_signal_lib():
    """The mGru models' first layer, 1 -> Cout channels on the raw signal (include/taiyaki_amd_conv_signal.h).  No
    fallback: a missing library raises."""
    return _load(os.path.join(CSRC, CONV_SIGNAL_LIBNAME), CONV_SIGNAL_SIGNATURES)


def out_layer_lib():
    """The models' output layer, plain and cat-mod (include/taiyaki_amd_out_layer.h): the lab build of that library
    while the process runs on the lab build (`use_lab`), the release one otherwise.  No fallback: a missing library
    raises."""
    if is_lab():
        return _load(os.path.join(CSRC, OUT_LAYER_LAB_LIBNAME),
                     dict(OUT_LAYER_SIGNATURES, **OUT_LAYER_LAB_SIGNATURES))
    return _load(os.path.join(CSRC, OUT_LAYER_LIBNAME), OUT_LAYER_SIGNATURES)


def conv_window_lib():
    """The 16 -> Cout convolution at the fast and the RNA models' shapes (include/taiyaki_amd_conv_window.h): the lab
    build of that library while the process runs on the lab build (`use_lab`), the release one otherwise.  No fallback:
    a missing library raises."""
    if is_lab():
        return _load(os.path.join(CSRC, CONV_WINDOW_LAB_LIBNAME),
                     dict(CONV_WINDOW_SIGNATURES, **CONV_WINDOW_LAB_SIGNATURES))
    return _load(os.path.join(CSRC, CONV_WINDOW_LIBNAME), CONV_WINDOW_SIGNATURES)


def chunks_seqlen_lib():
    """Chunks of a fixed number of bases and the squiggle trainer's batch of them (include/taiyaki_amd_chunks_seqlen.h).
    No fallback: a missing library raises."""
    return _load(os.path.join(CSRC, CHUNKS_SEQLEN_LIBNAME), CHUNKS_SEQLEN_SIGNATURES)


def optim_lib():
    """The optimiser step over the flat gradient arena (include/taiyaki_amd_optim.h).  No fallback: a missing library
    raises."""
    return _load(os.path.join(CSRC, OPTIM_LIBNAME), OPTIM_SIGNATURES)


def varlen_lib():
    """The recurrences' forward with per-column lengths (include/taiyaki_amd_rnn_varlen.h).  No fallback: a missing
    library raises."""
    return _load(os.path.join(CSRC, VARLEN_LIBNAME), VARLEN_SIGNATURES)


def varlen_train_lib():
    """The recurrences' training pair with per-column lengths (include/taiyaki_amd_rnn_varlen_train.h).  No fallback: a
    missing library raises."""
    return _load(os.path.join(CSRC, VARLEN_TRAIN_LIBNAME), VARLEN_TRAIN_SIGNATURES)


def rnn_wide_lib():
    """The recurrences at every batch width, as slabs of columns (include/taiyaki_amd_rnn_wide.h).  No fallback: a
    missing library raises."""
    return _load(os.path.join(CSRC, WIDE_LIBNAME), WIDE_SIGNATURES)


def decode_varlen_lib():
    """The decode operators with per-column lengths (include/taiyaki_amd_decode_varlen.h).  No fallback: a missing
    library raises."""
    return _load(os.path.join(CSRC, DECODE_VARLEN_LIBNAME), DECODE_VARLEN_SIGNATURES)


def loss_varlen_lib():
    """The flip-flop loss with a time length per column (include/taiyaki_amd_loss_varlen.h): loaded by the first call that
    brings lengths.  No fallback: a missing library raises."""
    return _load(os.path.join(CSRC, LOSS_VARLEN_LIBNAME), LOSS_VARLEN_SIGNATURES)


def check(rc, what):
    if rc != 0:
        raise RuntimeError("%s failed: %s (code %d)" % (what, ERRORS.get(rc, "unknown"), rc))


def require_gpu(t, what):
    if not t.is_cuda:
        raise RuntimeError(
            "%s: tensor is on %s; the flip-flop operators only run as HIP kernels on an AMD GPU "
            "(no CPU fallback)" % (what, t.device))


def ptr(t):
    return _vp(t.data_ptr()) if t is not None else _vp(0)


def stream_ptr():
    return _vp(torch.cuda.current_stream().cuda_stream)


# --------------------------------------------------------------------------
# scratch memory of the kernels
# --------------------------------------------------------------------------
_WS_CACHE = {}


def workspace(nbytes, dev, tag, fresh=False):
    """The kernels' scratch memory.  Eager calls reuse ONE buffer per (device, stream, operator
    slot `tag`), grown when a call needs more -- calls on a stream are ordered, so nothing that is
    still being read is handed out again -- instead of a `torch.empty` of up to gigabytes per call.
    While a hipGraph is being captured (or `fresh`) the buffer is allocated anew: it then belongs
    to the graph's private pool and lives as long as the graph."""
    if fresh or torch.cuda.is_current_stream_capturing():
        return torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
    key = (dev.index, torch.cuda.current_stream(dev).cuda_stream, tag)
    buf = _WS_CACHE.get(key)
    if buf is None or buf.numel() < nbytes:
        if len(_WS_CACHE) > 64:
            _WS_CACHE.clear()
        _WS_CACHE.pop(key, None)            # (release the old one before asking for the larger one)
        buf = None
        buf = _WS_CACHE[key] = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
    return buf


def release_workspaces():
    """Drop the cached scratch buffers (they are re-created on demand)."""
    _WS_CACHE.clear()


# --------------------------------------------------------------------------
# non-finite reporting (reference: AssertionError in ctc.pyx:48,62-65,107-112)
# --------------------------------------------------------------------------
_strict = os.environ.get("TAIYAKI_AMD_STRICT", "1") != "0"
_deferred = {}


def is_strict():
    return _strict


def set_strict(flag):
    """strict (default): every operator call checks its device status word at once
    (one host sync, exactly the reference's error timing).  Non-strict: status
    words accumulate per device and are checked by `raise_if_nonfinite()`."""
    global _strict
    _strict = bool(flag)


def status_word(device):
    if _strict:
        return torch.zeros(1, dtype=torch.int32, device=device)
    key = (device.type, device.index)
    if key not in _deferred:
        _deferred[key] = torch.zeros(1, dtype=torch.int32, device=device)
    return _deferred[key]


_gated = {"last": 0, "total": 0, "last_retried": 0, "total_retried": 0}
_COUNT_MASK, _GATED_SHIFT, _RETRIED_SHIFT = (DEFINES["TK_STATUS_" + k] for k in ("COUNT_MASK", "GATED_SHIFT", "RETRIED_SHIFT"))


def last_gate_count():
    """Reads that the CRF's linear-domain path handed to its log-domain kernel (status word bits
    8-19, include/taiyaki_amd_flipflop.h): in strict mode of the most recent operator call, in
    non-strict mode between the last two `raise_if_nonfinite()` / `take_gate_count()` checks.
    Such reads are RIGHT but cost ~1000x a read on the linear path (1 ms at T = 800): a batch that
    keeps producing them (scores far outside the network's 5 tanh range, violent cat-mod logits)
    is losing time."""
    return _gated["last"]


def last_retry_count():
    """Reads that the batch's launch of the CRF's linear path disowned and the retry launch swept again,
    alone and at its conservative configuration (status word bits 20-31; round 6) -- counted like
    `last_gate_count`, which says how many of them failed there too.  A retried read costs about what
    two reads cost the batch's launch."""
    return _gated["last_retried"]


def _u32(bits):
    """The status words are int32 tensors; the kernels add their counts into bits 8-31 (unsigned)."""
    return int(bits) & 0xffffffff


def _counts(bits):
    return (bits >> _GATED_SHIFT) & _COUNT_MASK, (bits >> _RETRIED_SHIFT) & _COUNT_MASK


def _note(redone, retried):
    _gated["last"], _gated["last_retried"] = redone, retried
    _gated["total"] += redone
    _gated["total_retried"] += retried


def _note_gated(bits):
    bits = _u32(bits)
    _note(*_counts(bits))
    return int(bits) & 0xff


def take_gate_count():
    """Non-strict mode: read and clear the COUNTS of the deferred status words (one sync per
    device), leaving the error flags to `raise_if_nonfinite()`.  Returns the number of reads
    redone in the log domain since the last check (`last_retry_count()`: the reads retried)."""
    n = m = 0
    for t in _deferred.values():
        bits = _u32(t.item())
        redone, retried = _counts(bits)
        n, m = n + redone, m + retried
        if bits >> 8:
            # take out exactly what was read (one device op, wrap-around arithmetic): counts that kernels on
            # other streams add between the read and this op are kept, not cleared with the rest
            take = (bits >> 8) << 8
            t.sub_(take - (1 << 32) if take >= (1 << 31) else take)
    _note(n, m)
    return n


def gated_total():
    """Reads redone in the log domain since the process started, as far as the status words have
    been read (every call in strict mode; at `raise_if_nonfinite()` / `take_gate_count()` otherwise)."""
    return _gated["total"]


def retried_total():
    return _gated["total_retried"]


def _raise(bits):
    bits = _u32(bits) & 0xff
    if bits & 64:
        # the reference asserts nsample > 0 (c_squiggle_match.c:112) and reads past the signal otherwise
        raise ValueError("squiggle match: a siglen is <= 0, or sum(siglen) exceeds len(signal)")
    if bits & 8:
        # the reference: `assert np.all(stayidxs >= 0) and ...` style index checks in ctc.pyx
        raise AssertionError("Error: sequence labels out of range for the flip-flop model (flip-flop code "
                             "outside [0, 2 nbase), modification category outside its base's range, or "
                             "sum(seqlen) larger than the label array)")
    if bits & 32:
        raise RuntimeError("LSTM / GRU recurrence: a workgroup waited past its time budget for the rest of its group "
                           "(the layer's outputs are not valid)")
    if bits & 16:
        raise RuntimeError("a sequence is longer than the max_seqlen the CRF kernel was launched for")
    if bits & 4:
        raise RuntimeError("sequence buffer overflow: a chunk batch needed more than max_bases_per_chunk bases "
                           "per chunk (its `seqs` would be truncated)")
    if bits & 1:
        raise AssertionError("Error: all costs must be finite.\n"
                             "Try restarting from a checkpoint with a lower learning rate.")
    if bits & 2:
        raise AssertionError("Error: Gradients not finite.\n"
                             "Try restarting from a checkpoint with a lower learning rate.")


def finish(status):
    if _strict:
        _raise(_note_gated(int(status.item())))


def raise_if_nonfinite():
    """Check (and clear) the deferred status words; one sync per device."""
    total, retried, first_bad = 0, 0, 0
    for t in _deferred.values():
        bits = _u32(t.item())
        t.zero_()
        redone, again = _counts(bits)
        total, retried = total + redone, retried + again
        first_bad = first_bad or (bits & 0xff)
    _note(total, retried)
    _raise(first_bad)
