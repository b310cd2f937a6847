"""ctypes binding of libb4c_hip.so (include/b4c.h).  There is no CPU fallback: if the
library is missing, or a call fails, this raises -- the product path is the HIP path."""
import ctypes
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('B4C_LIB_PATH') or os.path.join(_HERE, 'libb4c_hip.so')     # override: A/B of two builds (scratch)
HEADER_PATH = os.path.join(os.path.dirname(_HERE), 'include', 'b4c.h')      # the whole ABI (B4C_ABI_VERSION): the one header, read when lib() binds


class B4CError(RuntimeError):
    pass


class PackDesc(ctypes.Structure):
    """b4c_pack_desc of include/b4c.h."""
    _fields_ = [('src', ctypes.c_void_p), ('bias_src', ctypes.c_void_p), ('wt', ctypes.c_void_p), ('wc', ctypes.c_void_p),
                ('bias_dst', ctypes.c_void_p), ('K', ctypes.c_int32), ('N', ctypes.c_int32), ('ld_t', ctypes.c_int32),
                ('ld_c', ctypes.c_int32), ('col_off', ctypes.c_int32), ('_pad', ctypes.c_int32)]


class TNDesc(ctypes.Structure):
    """b4c_tn_desc of include/b4c.h."""
    _fields_ = [('A', ctypes.c_void_p), ('G', ctypes.c_void_p), ('dW', ctypes.c_void_p * 4), ('db', ctypes.c_void_p * 4),
                ('lda', ctypes.c_int32), ('ldg', ctypes.c_int32), ('K', ctypes.c_int32), ('n_seg', ctypes.c_int32),
                ('seg_width', ctypes.c_int32), ('ldw', ctypes.c_int32)]


# The header is the one place a signature or a constant is written: the binding below is derived from its text.
_CTYPES = {'int': ctypes.c_int, 'int32_t': ctypes.c_int, 'int64_t': ctypes.c_int64, 'float': ctypes.c_float,
           'uint64_t': ctypes.c_uint64, 'uint32_t': ctypes.c_uint32}


def _header_text(header_path):
    """include/b4c.h without its comments"""
    try:
        with open(header_path) as f:
            return re.sub(r'/\*.*?\*/', '', f.read(), flags=re.S)
    except OSError as e:
        raise B4CError('cannot read the C header %s (%s): the binding is derived from it' % (header_path, e)) from None


def _ctype(text, decl, is_return=False):
    """ctypes type of one parameter (`const float *bias`, `int64_t M`) or return type.  Every pointer argument is c_void_p,
    the HOST arrays (h_ids, h_dims, ...) too: c_void_p takes the ctypes arrays the callers build ((c_void_p * n)(...),
    (c_int * n)(...)) as well as None and integers, where a typed POINTER would also check the element type."""
    words = re.findall(r'\w+|\*', text)
    if '*' in words:
        if not is_return:
            return ctypes.c_void_p
        if words == ['const', 'char', '*']:
            return ctypes.c_char_p
    else:
        words = [w for w in words if w != 'const']
        if len(words) == (1 if is_return else 2) and words[0] in _CTYPES:      # (a parameter: its type and its name)
            return _CTYPES[words[0]]
    raise B4CError('include/b4c.h: unknown type %r in the declaration %r' % (' '.join(text.split()), decl))


def parse_header(src):
    """{name: (restype, [argtypes])} of every function the header text `src` (comments removed) declares.  Anything between two
    `;` that is not a function declaration of known types raises: a skipped or guessed argument would shift all that follow."""
    src = re.sub(r'^[ \t]*#.*$', '', src, flags=re.M)                                   # preprocessor lines
    src = re.sub(r'typedef\s+struct\s*\{[^}]*\}\s*\w+\s*;', '', src)                   # b4c_pack_desc, b4c_tn_desc: PackDesc, TNDesc
    src = re.sub(r'extern\s+"C"\s*\{|^\s*\}\s*$', '', src, flags=re.M)
    table = {}
    for decl in src.split(';'):
        decl = ' '.join(decl.split())
        if not decl:
            continue
        m = re.fullmatch(r'(.*?)\b(\w+) ?\(([^()]*)\)', decl)
        if not m or not m.group(1).strip():
            raise B4CError('include/b4c.h: cannot parse the declaration %r' % decl)
        if m.group(2) in table:                      # (the one duplicate check of the ABI: one header, one table)
            raise B4CError('include/b4c.h declares %s twice: %r' % (m.group(2), decl))
        ret, name, args = m.groups()
        args = [] if args.strip() == 'void' else [_ctype(a, decl) for a in args.split(',')]
        table[name] = (_ctype(ret, decl, True), args)
    return table


def header_constants(src):
    """{name: value} of the header's integer #defines (B4C_F32, B4C_MAX_TOPK, B4C_EINVAL, B4C_ATTN_CAUSAL 1u, ...)"""
    return {k: int(v) for k, v in re.findall(r'^[ \t]*#[ \t]*define[ \t]+(B4C_\w+)[ \t]+\(?(-?\d+)[uU]?\)?[ \t]*$', src, flags=re.M)}


def signatures(header_path=HEADER_PATH):
    """{name: (restype, [argtypes])} of every entry point include/b4c.h declares: the whole ABI, and what lib() binds."""
    return parse_header(_header_text(header_path))


def declared_symbols(header_path=HEADER_PATH):
    """Names of every function include/b4c.h declares (build() and the symbol-export test compare them with the library's exports)."""
    return sorted(signatures(header_path))


_C = header_constants(_header_text(HEADER_PATH))
ABI_VERSION = _C['B4C_ABI_VERSION']       # b4c_abi_version() of the library must agree
F32, BF16 = _C['B4C_F32'], _C['B4C_BF16']
ACT_NONE, ACT_RELU = _C['B4C_ACT_NONE'], _C['B4C_ACT_RELU']
ACT_GELU, ACT_GELU_TANH = _C['B4C_ACT_GELU'], _C['B4C_ACT_GELU_TANH']
CE_TF, CE_PLAIN = _C['B4C_CE_TF'], _C['B4C_CE_PLAIN']
MAX_FEATURES, MAX_TOPK = _C['B4C_MAX_FEATURES'], _C['B4C_MAX_TOPK']
MAX_EXCL, MAX_CAND = _C['B4C_MAX_EXCL'], _C['B4C_MAX_CAND']
MAX_BATCH_WIDTH, MAX_CLOZE_LABELS = _C['B4C_MAX_BATCH_WIDTH'], _C['B4C_MAX_CLOZE_LABELS']      # limits of the device-built batches
GRAD_CHUNK, GRAD_GROUP = _C['B4C_GRAD_CHUNK'], _C['B4C_GRAD_GROUP']
ATTN_CAUSAL = _C['B4C_ATTN_CAUSAL']       # flag bit of the b4c_attn_*_ex entry points
CAND_BCE, CAND_SOFTMAX = _C['B4C_CAND_BCE'], _C['B4C_CAND_SOFTMAX']      # loss kinds of b4c_candidate_loss_fwd
CANDX_BCE, CANDX_SOFTMAX, CANDX_BPR = _C['B4C_CANDX_BCE'], _C['B4C_CANDX_SOFTMAX'], _C['B4C_CANDX_BPR']      # of b4c_candidate_loss_fwd_ex
CANDX_KINDS, CANDX_CORR_TARGET = _C['B4C_CANDX_KINDS'], _C['B4C_CANDX_CORR_TARGET']      # (CORR_TARGET: its flags bit)
NEXT_TRAIN, NEXT_EVAL = _C['B4C_NEXT_TRAIN'], _C['B4C_NEXT_EVAL']        # modes of b4c_next_item_batch
NEXT_EXCL_NONE, NEXT_EXCL_HISTORY = _C['B4C_NEXT_EXCL_NONE'], _C['B4C_NEXT_EXCL_HISTORY']
FEAT_EVENT, FEAT_ITEM = _C['B4C_FEAT_EVENT'], _C['B4C_FEAT_ITEM']        # source kinds of b4c_batch_features
FEAT_MASKED, FEAT_KEPT = _C['B4C_FEAT_MASKED'], _C['B4C_FEAT_KEPT']      # what a [MASK] position of the item row does to a feature
FEAT_CLOZE, FEAT_NEXT_TRAIN, FEAT_NEXT_EVAL = _C['B4C_FEAT_CLOZE'], _C['B4C_FEAT_NEXT_TRAIN'], _C['B4C_FEAT_NEXT_EVAL']      # row layouts
NCE_COSINE, NCE_MAX_N = _C['B4C_NCE_COSINE'], _C['B4C_NCE_MAX_N']        # the in-batch contrastive loss (b4c_nce_fwd / _bwd)
AUG_CROP, AUG_MASK, AUG_REORDER, AUG_SAME_TARGET = _C['B4C_AUG_CROP'], _C['B4C_AUG_MASK'], _C['B4C_AUG_REORDER'], _C['B4C_AUG_SAME_TARGET']
AUG_MAX_VIEWS = _C['B4C_AUG_MAX_VIEWS']      # (the ops_mask bits and the view limit of b4c_augment_views)
ATTN_LONG_MAX_S = _C['B4C_ATTN_LONG_MAX_S']      # longest sequence of b4c_attn_long_fwd / _bwd

_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise B4CError(
                'libb4c_hip.so not found at %s: build it with `python -c "import __graft_entry__ as g; g.build()"` '
                '(or `make -C bert4clickpath_amd/csrc`).  There is no CPU fallback.' % LIB_PATH)
        # PyTorch's HIP runtime must have seen the device before this library (and the system HIP runtime it links)
        # comes into the process: loaded the other way round -- e.g. build() and then smoke() in ONE process -- this
        # library's launches fail with "no ROCm-capable device is detected".  (No GPU: nothing to initialise.)
        try:
            import torch
            if torch.cuda.is_available():
                torch.cuda.init()
        except ImportError:
            pass
        L = ctypes.CDLL(LIB_PATH)
        sig = signatures(HEADER_PATH)        # (the module's HEADER_PATH now, not the default bound when signatures was defined)
        # The argument lists of the header belong to ONE ABI version: a library that exports the same names with older lists would
        # take a device pointer for a stream and fault on the GPU.  Compare before anything is bound.
        try:
            L.b4c_abi_version.restype = ctypes.c_int
            have = int(L.b4c_abi_version())
        except AttributeError:
            raise B4CError('%s does not export b4c_abi_version: not a libb4c_hip.so of this tree; rebuild it '
                           '(`make -C bert4clickpath_amd/csrc`)' % LIB_PATH) from None
        if have != ABI_VERSION:
            raise B4CError('%s is ABI %d, this binding expects ABI %d; rebuild it (`make -C bert4clickpath_amd/csrc`)'
                           % (LIB_PATH, have, ABI_VERSION))
        for name, (res, args) in sig.items():
            try:
                fn = getattr(L, name)
            except AttributeError:
                raise B4CError('%s (ABI %d) does not export %s; rebuild it (`make -C bert4clickpath_amd/csrc`)'
                               % (LIB_PATH, have, name)) from None
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def check(rc, what=''):
    if rc != 0:
        raise B4CError('%s failed (rc=%d): %s' % (what or 'b4c call', rc, lib().b4c_last_error().decode()))
