"""ctypes binding of the mmseq C ABI (include/mmseq.h) — the only path to the HIP kernels.

The header is the one statement of the ABI: at import `parse_header` reads every prototype's
argument types, the enum / #define constants and the two by-value structs from it, so nothing here
restates a signature. Status-returning entries go through `_call`, which names the entry once and
appends torch's current stream (every such entry takes it last).

There is deliberately no fallback: if `_lib/libmmseq.so` is missing or a kernel returns an
error, the call raises. Every wrapper takes torch tensors that already live on the current HIP
device and launches on torch's current stream.
"""
import ctypes
import math
import os
import re

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "_lib", "libmmseq.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "mmseq.h")

_vp = ctypes.c_void_p


class Rows(ctypes.Structure):
    """mmseq_rows: row r at base + (r // rpb) * bstride + (r % rpb) * ld (elements)."""
    _fields_ = [("ld", ctypes.c_int64), ("bstride", ctypes.c_int64), ("rpb", ctypes.c_int64)]


def rows(ld, bstride=0, rpb=1 << 62):
    return Rows(ld, bstride, rpb)


class Dropout(ctypes.Structure):
    """mmseq_dropout: counter-based mask keyed by (seed, stream, element index)."""
    _fields_ = [("p", ctypes.c_float), ("stream", ctypes.c_uint32), ("seed", ctypes.c_uint64)]


_dp = ctypes.POINTER(Dropout)


def drop(p, stream, seed):
    """A dropout descriptor, or None when p == 0 (the kernels then skip the mask)."""
    return Dropout(p, stream & 0xFFFFFFFF, seed & 0xFFFFFFFFFFFFFFFF) if p > 0 else None


def _d(d):
    return None if d is None else ctypes.byref(d)


class NativeError(RuntimeError):
    pass


# By-value C types of the header -> ctypes; parse_header adds the header's own enum / int typedefs.
_SCALARS = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "float": ctypes.c_float,
            "double": ctypes.c_double, "uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64,
            "mmseq_stream": _vp, "mmseq_rows": Rows}
_RETURNS = {"mmseq_status": ctypes.c_int, "int64_t": ctypes.c_int64, "const char*": ctypes.c_char_p}


def parse_header(text):
    """The text of mmseq.h -> (signatures: name -> (restype, [argtypes]), constants: NAME -> int
    for every enumerator and every `#define MMSEQ_NAME <integer>`, structs: typedef name ->
    [(field, ctype)]). A declaration or a type it does not know raises NativeError: nothing
    defaults to int."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    scalars = dict(_SCALARS)

    def take(pattern):
        """The groups of every match of a statement pattern; the statements leave the text."""
        nonlocal text
        found = re.findall(pattern, text, flags=re.M)
        text = re.sub(pattern, " ", text, flags=re.M)
        return found

    def scalar(decl, where):
        """The ctype of the by-value declaration `[const] <type> [name]`."""
        toks = [t for t in decl.split() if t != "const"]
        if not 1 <= len(toks) <= 2 or toks[0] not in scalars:
            raise NativeError(f"mmseq.h: unknown type in {' '.join(decl.split())!r} ({where})")
        return scalars[toks[0]]

    consts = {name: int(v, 0) for name, v in
              take(r"^[ \t]*#[ \t]*define[ \t]+(MMSEQ_\w+)[ \t]+(-?(?:0[xX][0-9a-fA-F]+|\d+))[ \t]*$")}
    take(r'^[ \t]*#[^\n]*|extern\s+"C"\s*\{|typedef\s+struct\s+\w+\s*\*\s*mmseq_stream\s*;')
    for name in take(r"typedef\s+int\s+(\w+)\s*;"):
        scalars[name] = ctypes.c_int
    for body, name in take(r"(?:typedef\s+)?enum\s*\{([^}]*)\}\s*(\w*)\s*;"):
        if name:
            scalars[name] = ctypes.c_int
        for item in filter(str.strip, body.split(",")):
            e = re.fullmatch(r"\s*(\w+)\s*=\s*(-?\w+)\s*", item)
            if not e:
                raise NativeError(f"mmseq.h: cannot parse enumerator {item.strip()!r}")
            consts[e[1]] = int(e[2], 0)
    structs = {name: [(f.split()[-1], scalar(f, name)) for f in filter(str.strip, body.split(";"))]
               for body, name in take(r"typedef\s+struct\s*\{([^}]*)\}\s*(\w+)\s*;")}
    sigs = {}
    for decl in filter(None, (d.strip() for d in text.split(";"))):
        if decl == "}":  # closes extern "C"
            continue
        m = re.fullmatch(r"(mmseq_status|int64_t|const\s+char\s*\*)\s*(mmseq_\w+)\s*\(([^()]*)\)", decl)
        if not m:
            raise NativeError(f"mmseq.h: cannot parse declaration {' '.join(decl.split())!r}")
        args = [] if m[3].strip() in ("", "void") else m[3].split(",")
        sigs[m[2]] = (_RETURNS[re.sub(r"\s*\*", "*", " ".join(m[1].split()))],
                      [(_dp if re.search(r"\bmmseq_dropout\b", a) else _vp) if "*" in a
                       else scalar(a, m[2]) for a in args])
    return sigs, consts, structs


def _read_header():
    if not os.path.exists(HEADER_PATH):
        raise NativeError(f"mmseq C header not found at {HEADER_PATH}; the binding reads every "
                          "signature and constant from it.")
    with open(HEADER_PATH) as f:
        return f.read()


# name -> (restype, argtypes); NAME -> value; typedef name -> fields
_SIGS, CONSTANTS, STRUCTS = parse_header(_read_header())

F32, BF16 = CONSTANTS["MMSEQ_F32"], CONSTANTS["MMSEQ_BF16"]
ACT = {"none": CONSTANTS["MMSEQ_ACT_NONE"], "gelu": CONSTANTS["MMSEQ_ACT_GELU_ERF"],
       "quickgelu": CONSTANTS["MMSEQ_ACT_QUICKGELU"], "tanh": CONSTANTS["MMSEQ_ACT_TANH"],
       "gelu_tanh": CONSTANTS["MMSEQ_ACT_GELU_TANH"]}
EUNSUPPORTED = CONSTANTS["MMSEQ_EUNSUPPORTED"]
XENT_EVAL_MAX_K = CONSTANTS["MMSEQ_XENT_EVAL_MAX_K"]

# Split-K slab workspaces, one per (device, stream): the C ABI takes the workspace per call and
# only work enqueued on that stream touches it, so calls on different streams never share one.
WORKSPACE_BYTES = 256 << 20
_ws = {}


def gemm_workspace(device, stream=None):
    dev = torch.device(device)
    if stream is None:
        stream = torch.cuda.current_stream(dev)
    key = (dev.index if dev.index is not None else torch.cuda.current_device(), stream.cuda_stream)
    buf = _ws.get(key)
    if buf is None:
        buf = _ws[key] = torch.empty(WORKSPACE_BYTES // 4, dtype=torch.float32, device=dev)
    return buf


# Per-call kernel selection (include/mmseq.h mmseq_gemm_variant / attention variant). The
# defaults below are what the product path uses; tests and microbenchmarks switch them with
# gemm_set_fast / attn_set_fast (Python-side defaults only: the C ABI holds no selection state).
GEMM_AUTO = CONSTANTS["MMSEQ_GEMM_AUTO"]
_sel = {"gemm": GEMM_AUTO, "attn": 1}
_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise NativeError(
                f"mmseq HIP library not found at {LIB_PATH}; run __graft_entry__.build() "
                "(make -C multimodal_sequencing_amd/csrc). There is no CPU fallback.")
        L = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in _SIGS.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def _check(st, what):
    if st != 0:
        raise NativeError(f"{what} failed ({st}): {lib().mmseq_last_error().decode()}")


def _status(st, name):
    """The tail of the decoder wrappers: MMSEQ_EUNSUPPORTED comes back as the status (the caller
    decides what to do instead), every other failure raises."""
    if st != EUNSUPPORTED:
        _check(st, name)
    return st


class Unsupported(NativeError):
    """An entry point returned MMSEQ_EUNSUPPORTED: nothing was launched."""
    status = EUNSUPPORTED


def _check_shape(st, what):
    if st == EUNSUPPORTED:
        raise Unsupported(f"{what}: unsupported shape: {lib().mmseq_last_error().decode()}")
    _check(st, what)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _raw(name, *args):
    """The mmseq_status of a status-returning entry; torch's current stream is appended."""
    return getattr(lib(), name)(*args, _stream())


def _call(name, *args, tail=_check):
    """One call of a status-returning entry; a nonzero status goes to `tail`: _check (raise on any
    failure), _status (return MMSEQ_EUNSUPPORTED) or _check_shape (raise Unsupported for it).
    Every wrapper of the training step passes here: _raw's line is repeated, and MMSEQ_OK returns
    at once, to keep a call at the three Python frames it had with the entry spelled out."""
    st = getattr(lib(), name)(*args, _stream())
    return st if st == 0 else tail(st, name)


def _p(t):
    return None if t is None else t.data_ptr()


def dt(t):
    if t.dtype == torch.float32:
        return F32
    if t.dtype == torch.bfloat16:
        return BF16
    raise NativeError(f"unsupported dtype {t.dtype}")


def _dev(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise NativeError("mmseq kernels need device tensors (no CPU fallback)")


def _expect(what, *checks):
    """Every (tensor, dtype, shape) is a contiguous device tensor of that dtype and shape (an int
    for `shape`: that many elements in any shape), else ValueError (NativeError off the device)."""
    for t, dtype, shape in checks:
        ok = torch.is_tensor(t) and t.dtype == dtype and t.is_contiguous() and \
            (t.numel() == shape if isinstance(shape, int) else tuple(t.shape) == tuple(shape))
        if not ok:
            want = f"[{shape}]" if isinstance(shape, int) else tuple(shape)
            got = f"{tuple(t.shape)} {t.dtype}" if torch.is_tensor(t) else type(t).__name__
            raise ValueError(f"{what}: contiguous {dtype} {want} expected, got {got}")
        _dev(t)


class MXFP8:
    """An MX-fp8 operand: q uint8 [rows][K] (OCP e4m3 bits) + packed E8M0 scales."""
    __slots__ = ("q", "scales", "rows", "K")

    def __init__(self, q, scales, rows, K):
        self.q, self.scales, self.rows, self.K = q, scales, rows, K

    @classmethod
    def alloc(cls, rows, K, device, zero_scales):
        """Output buffers of a producer: q [rows][K rounded up to 16] and the scale bytes.
        zero_scales: for the producers that leave the padding rows' scales to the caller."""
        q = torch.empty(rows, (K + 15) // 16 * 16, dtype=torch.uint8, device=device)
        new = torch.zeros if zero_scales else torch.empty
        return cls(q, new(lib().mmseq_mxfp8_scale_bytes(rows, K), dtype=torch.uint8, device=device),
                   rows, K)


# ------------------------------------------------------------------------------------------------
def gemm(A, B, C, M, N, K, *, trans=0, lda=None, ldb=None, ldc=None, batch=1, sA=0, sB=0, sC=0,
         bias=None, act=0, aux=None, dact=None, resid=None, ldr=None, sR=0, alpha=1.0,
         accumulate=False, drop=None):
    _dev(A, B, C)
    ws = gemm_workspace(A.device)
    if lda is None:
        lda = M if trans else K
    if ldb is None:
        ldb = N if trans else K
    if ldc is None:
        ldc = N
    if ldr is None:
        ldr = ldc
    _call("mmseq_gemm", trans, M, N, K, batch, _p(A), lda, sA, _p(B), ldb, sB, _p(C), ldc, sC,
          _p(bias), act, _p(aux), _p(dact), _p(resid), ldr, sR, alpha, int(accumulate), dt(A), dt(C),
          _d(drop), _sel["gemm"], ws.data_ptr(), ws.numel() * 4)


def gemm_wgrad(dy, x, gW, gb=None, lddy=None):
    """gW[out][in] += dy^T x and gb[out] += column sums of dy (fp32), dy [R][out], x [R][in]. With
    lddy, dy is [R][>= out] with that row stride (a column range of a wider, row-padded buffer)."""
    _dev(dy, x, gW)
    ws = gemm_workspace(dy.device)
    M, Nn = gW.shape
    R = x.numel() // x.shape[-1]
    if lddy is None:
        lddy = dy.shape[-1]
    _call("mmseq_gemm_wgrad", M, Nn, R, _p(dy), lddy, _p(x), x.shape[-1], _p(gW), Nn, _p(gb), dt(dy),
          _sel["gemm"], ws.data_ptr(), ws.numel() * 4)


def gemm_set_fast(variant):
    """Default GEMM variant passed by this binding (mmseq_gemm_variant): 1 = auto (product),
    2 = 128^2 double-buffer, 3 = 128^2 ring, 4 = 256^2 NT always, 5 = 256x128 NT, 6 = 256x128 NT
    ping-pong (two 4-wave groups per CU), 0 = generic."""
    _sel["gemm"] = int(variant)


def attn_set_fast(variant):
    """bf16 attention variant passed by this binding: 1 = 128-row 16x16x32 LDS-DMA pipelined
    kernels (product), 2 = 32x32x16-MFMA forward (measured, not faster), 0 = the 64-row kernels
    (cross-checks in the tests). The backward uses the 128-row kernels for any nonzero variant."""
    _sel["attn"] = int(variant)


def attn_fwd(P, T, heads, qkv, ld_qkv, q_off, k_off, v_off, key_bias, scale, out, ld_out, lse,
             drop=None, keep_bits=None):
    _dev(qkv, out, lse)
    _call("mmseq_attn_fwd", P, T, heads, _p(qkv), ld_qkv, q_off, k_off, v_off, _p(key_bias), scale,
          _p(out), ld_out, _p(lse), dt(qkv), _d(drop), _p(keep_bits), _sel["attn"])


def attn_keep_bits(P, T, heads, device):
    """Buffer for the forward's attention-dropout keep mask as bits (read back by attn_bwd)."""
    return torch.empty(lib().mmseq_attn_keep_bits_words(P, T, heads), dtype=torch.int64,
                       device=device)


def attn_bwd(P, T, heads, qkv, ld_qkv, q_off, k_off, v_off, key_bias, scale, out, ld_out, dout,
             ld_dout, lse, delta, dqkv, ld_dqkv, drop=None, keep_bits=None):
    _call("mmseq_attn_bwd", P, T, heads, _p(qkv), ld_qkv, q_off, k_off, v_off, _p(key_bias), scale,
          _p(out), ld_out, _p(dout), ld_dout, _p(lse), _p(delta), _p(dqkv), ld_dqkv, dt(qkv),
          _d(drop), _p(keep_bits), _sel["attn"])


def attn_fwd_rows(P, T, Tq, heads, qkv, key_bias, scale, out, lse, drop=None, keep_bits=None):
    """The bf16 forward for queries 0 .. Tq-1 of every sequence (packed Q|K|V qkv [P*T][3H]):
    out [P*Tq][H], lse [P][heads][T] (rows < Tq), keep bits in mmseq_attn_fwd's layout."""
    _dev(qkv, out, lse)
    H = heads * 64
    _call("mmseq_attn_fwd_rows", P, T, Tq, heads, _p(qkv), 3 * H, 0, H, 2 * H, _p(key_bias), scale,
          _p(out), H, _p(lse), _d(drop), _p(keep_bits))


def attn_bwd_rows(P, T, Tq, heads, qkv, key_bias, scale, out, dout, lse, delta, dqkv, drop=None,
                  keep_bits=None):
    """Backward of attn_fwd_rows: out / dout [P*Tq][H]; dqkv [P*T][3H] (dQ = 0 on rows >= Tq)."""
    _dev(qkv, out, dout, dqkv)
    H = heads * 64
    _call("mmseq_attn_bwd_rows", P, T, Tq, heads, _p(qkv), 3 * H, 0, H, 2 * H, _p(key_bias), scale,
          _p(out), H, _p(dout), H, _p(lse), _p(delta), _p(dqkv), 3 * H, _d(drop), _p(keep_bits))


def small_attn_fwd(B, T, heads, d, q, k, v, key_bias, scale, out, probs, drop=None):
    _call("mmseq_small_attn_fwd", B, T, heads, d, _p(q), _p(k), _p(v), _p(key_bias), scale, _p(out),
          _p(probs), _d(drop))


def small_attn_bwd(B, T, heads, d, q, k, v, probs, dout, scale, dq, dk, dv, drop=None):
    _call("mmseq_small_attn_bwd", B, T, heads, d, _p(q), _p(k), _p(v), _p(probs), _p(dout), scale,
          _p(dq), _p(dk), _p(dv), _d(drop))


def layernorm_fwd(nrows, cols, x, xl, gamma, beta, eps, y, yl, mean, rstd, drop=None):
    _dev(x, y, gamma, beta)
    _call("mmseq_layernorm_fwd", nrows, cols, _p(x), xl, _p(gamma), _p(beta), eps, _p(y), yl,
          _p(mean), _p(rstd), dt(x), dt(y), _d(drop))


def layernorm_fwd_mxfp8(nrows, cols, x, gamma, beta, eps, y=None, mean=None, rstd=None):
    """LayerNorm of x [nrows][cols] bf16 (unit row stride layout) -> MXFP8 of the output (+ the bf16
    output into y when given) in one pass (mmseq_layernorm_fwd_mxfp8)."""
    _dev(x, gamma, beta)
    o = MXFP8.alloc(nrows, cols, x.device, zero_scales=False)
    _call("mmseq_layernorm_fwd_mxfp8", nrows, cols, _p(x), rows(cols), _p(gamma), _p(beta), eps,
          _p(y), rows(cols), _p(mean), _p(rstd), _p(o.q), o.q.stride(0), _p(o.scales))
    return o


def layernorm_bwd(nrows, cols, dy, dyl, x, xl, mean, rstd, gamma, dx, dxl, dres, dresl, dgamma,
                  dbeta, drop_dy=None, dx_drop=None, drop_dx=None, dx_drop_rows=None, dsum=None,
                  dsum_with_dres=False):
    """dx_drop_rows: the row layout of dx_drop (mmseq_layernorm_bwd_rows); default dx's. dsum:
    fp32 [cols] += column sums of the gradient written for the next GEMM (dx_drop, else dx) — the
    next Linear's bias gradient (mmseq_layernorm_bwd_ex). Without dx_drop that sum INCLUDES dres
    (dx = LN gradient + dres): a caller that means it (the CLIP out_proj, whose output gradient is
    exactly that) says so with dsum_with_dres=True; anyone else passing dres there is refused, so a
    BERT-style caller cannot fold a residual gradient into a bias gradient by accident."""
    ws = torch.empty(lib().mmseq_layernorm_bwd_workspace(nrows, cols), dtype=torch.float32,
                     device=x.device)
    if dsum is not None and dres is not None and dx_drop is None and not dsum_with_dres:
        raise ValueError("layernorm_bwd: dsum without dx_drop would sum dx INCLUDING dres; "
                         "pass dsum_with_dres=True if that is the bias gradient meant")
    # the three entries share their first 19 arguments
    head = (nrows, cols, _p(dy), dyl, _p(x), xl, _p(mean), _p(rstd), _p(gamma), _p(dx), dxl,
            _p(dres), dresl, _p(dgamma), _p(dbeta), _p(ws), dt(x), _d(drop_dy), _p(dx_drop))
    if dsum is not None:
        _dev(dsum)
        _call("mmseq_layernorm_bwd_ex", *head, dx_drop_rows if dx_drop_rows is not None else dxl,
              _d(drop_dx), _p(dsum))
    elif dx_drop_rows is not None:
        _call("mmseq_layernorm_bwd_rows", *head, dx_drop_rows, _d(drop_dx))
    else:
        _call("mmseq_layernorm_bwd", *head, _d(drop_dx))


def layernorm_bwd_mxfp8(nrows, cols, dy, dyl, x, xl, mean, rstd, gamma, dx, dxl, dres, dresl, dgamma,
                        dbeta, drop_dy=None, dx_drop=None, drop_dx=None):
    """layernorm_bwd (bf16) whose dgrad-GEMM operand (dx_drop, else dx) also leaves in MX-fp8
    (mmseq_layernorm_bwd_mxfp8) -> MXFP8 [nrows][cols]."""
    ws = torch.empty(lib().mmseq_layernorm_bwd_workspace(nrows, cols), dtype=torch.float32,
                     device=x.device)
    o = MXFP8.alloc(nrows, cols, x.device, zero_scales=True)
    _call("mmseq_layernorm_bwd_mxfp8", nrows, cols, _p(dy), dyl, _p(x), xl, _p(mean), _p(rstd),
          _p(gamma), _p(dx), dxl, _p(dres), dresl, _p(dgamma), _p(dbeta), _p(ws), _d(drop_dy),
          _p(dx_drop), _d(drop_dx), _p(o.q), o.q.stride(0), _p(o.scales))
    return o


def embed_ln_fwd(P, Lt, H, ids, tt, word, pos, typ, gamma, beta, eps, joint, ld_pair, mean, rstd,
                 drop=None):
    _call("mmseq_embed_ln_fwd", P, Lt, H, _p(ids), _p(tt), _p(word), _p(pos), _p(typ), _p(gamma),
          _p(beta), eps, _p(joint), ld_pair, _p(mean), _p(rstd), dt(joint), _d(drop))


def embed_ln_bwd(P, Lt, H, ids, tt, word, pos, typ, gamma, mean, rstd, djoint, ld_pair, dword,
                 dpos, dtyp, dgamma, dbeta, drop=None):
    ws = torch.empty(lib().mmseq_embed_ln_bwd_workspace(P, Lt, H), dtype=torch.float32,
                     device=djoint.device)
    _call("mmseq_embed_ln_bwd", P, Lt, H, _p(ids), _p(tt), _p(word), _p(pos), _p(typ), _p(gamma),
          _p(mean), _p(rstd), _p(djoint), ld_pair, _p(dword), _p(dpos), _p(dtyp), _p(dgamma),
          _p(dbeta), _p(ws), dt(djoint), _d(drop))


def vit_im2col(B, N, npair, R, ps, images, pairs, patches):
    """patches [rows][ld]: ld >= 3 ps^2, the extra columns are zero-filled."""
    _call("mmseq_vit_im2col", B, N, npair, R, ps, _p(images), _p(pairs), _p(patches),
          patches.shape[-1], dt(patches))


def vit_embed_fwd(P, ntok, W, npatch, patch_out, cls, pos, gamma, beta, eps, x, y, mean, rstd):
    _call("mmseq_vit_embed_fwd", P, ntok, W, npatch, _p(patch_out), _p(cls), _p(pos), _p(gamma),
          _p(beta), eps, _p(x), _p(y), _p(mean), _p(rstd), dt(x))


def vit_embed_bwd(P, ntok, W, npatch, dy, x, mean, rstd, gamma, dpatch, dcls, dpos, dgamma, dbeta):
    ws = torch.empty(lib().mmseq_vit_embed_bwd_workspace(P, ntok, W), dtype=torch.float32,
                     device=x.device)
    _call("mmseq_vit_embed_bwd", P, ntok, W, npatch, _p(dy), _p(x), _p(mean), _p(rstd), _p(gamma),
          _p(dpatch), _p(dcls), _p(dpos), _p(dgamma), _p(dbeta), _p(ws), dt(x))


def cast(src, dst):
    assert src.numel() == dst.numel()
    _call("mmseq_cast", src.numel(), _p(src), dt(src), _p(dst), dt(dst))


def transpose_cast_batch(desc, tiles, src, dst):
    """desc: int64 device tensor [n][5] = (rows, cols, src offset, dst offset, first 64x64 tile)
    of fp32 matrices in src (flat), transposed into dst (flat, dst's dtype)."""
    _dev(desc, src, dst)
    _call("mmseq_transpose_cast_batch", desc.shape[0], _p(desc), tiles, _p(src), _p(dst), dt(dst))


def transpose_cast(src, dst):
    r, c = src.shape
    _call("mmseq_transpose_cast", r, c, _p(src), _p(dst), dt(dst))


def colsum(x, nrows, cols, ldx, out, accumulate=True):
    ws = torch.empty(max(1, lib().mmseq_colsum_workspace(nrows, cols)), dtype=torch.float32,
                     device=x.device)
    _call("mmseq_colsum", nrows, cols, _p(x), ldx, _p(out), int(accumulate), _p(ws), dt(x))


def act_fwd(x, y, act):
    _call("mmseq_act_fwd", x.numel(), act, _p(x), _p(y), dt(x))


def act_bwd(z, dy, dz, act):
    _call("mmseq_act_bwd", z.numel(), act, _p(z), _p(dy), _p(dz), dt(z))


def dropout(x, y, drop):
    _call("mmseq_dropout_apply", x.numel(), _p(x), _p(y), dt(x), _d(drop))


def sumsq(x, out):
    ws = torch.empty(lib().mmseq_sumsq_workspace(x.numel()), dtype=torch.float32, device=x.device)
    _call("mmseq_sumsq", x.numel(), _p(x), _p(out), _p(ws))


def adamw(p, g, m, v, decay_mask, lr, b1, b2, eps, wd, step, max_norm, sumsq_buf, shadow):
    _call("mmseq_adamw", p.numel(), _p(p), _p(g), _p(m), _p(v), _p(decay_mask), lr, b1, b2, eps, wd,
          step, max_norm, _p(sumsq_buf), _p(shadow))


def pointer_fwd(B, N, H, q, key, okey, w, wb, pointed, tgt_len, target, logp, nll):
    _call("mmseq_pointer_fwd", B, N, H, _p(q), _p(key), _p(okey), _p(w), _p(wb), _p(pointed),
          _p(tgt_len), _p(target), _p(logp), _p(nll))


def pointer_bwd(B, N, H, q, key, okey, w, logp, pointed, tgt_len, target, dnll, dq, dkey, dokey,
                dw, dwb):
    ws = torch.empty(lib().mmseq_pointer_bwd_workspace(B, N, H), dtype=torch.float32, device=q.device)
    _call("mmseq_pointer_bwd", B, N, H, _p(q), _p(key), _p(okey), _p(w), _p(logp), _p(pointed),
          _p(tgt_len), _p(target), _p(dnll), _p(dq), _p(dkey), _p(dokey), _p(dw), _p(dwb), _p(ws))


def span_pool_fwd(P, Lt, H, top, ld_pair, score, sep, probs, mix, drop=None):
    _call("mmseq_span_pool_fwd", P, Lt, H, _p(top), ld_pair, _p(score), _p(sep), _p(probs), _p(mix),
          dt(top), _d(drop))


def span_pool_bwd(P, Lt, H, top, ld_pair, probs, sep, dmix, dscore, dtop, drop=None):
    _call("mmseq_span_pool_bwd", P, Lt, H, _p(top), ld_pair, _p(probs), _p(sep), _p(dmix),
          _p(dscore), _p(dtop), dt(top), _d(drop))


def pair_scan(input_ids, labels, cls_id, sep_id, starts, lens, plab, sep_pos, status):
    """status int32 [2], zeroed by the caller: (max pair length, malformed stories)."""
    B, L = input_ids.shape
    N = labels.shape[1]
    i64 = torch.int64
    _expect("pair_scan", (input_ids, i64, (B, L)), (labels, i64, labels.shape), (starts, i64, (B, N)),
            (lens, i64, (B, N)), (plab, i64, (B, N * (N - 1))), (sep_pos, i64, (B, N * (N - 1), 2)))
    if status.dtype != torch.int32 or status.numel() < 2:
        raise ValueError("pair_scan: status must be int32 [2]")
    _call("mmseq_pair_scan", B, L, N, _p(input_ids), _p(labels), cls_id, sep_id, _p(starts),
          _p(lens), _p(plab), _p(sep_pos), _p(status))


def pair_expand(input_ids, starts, lens, N, Lp, pad_id, second_type, out_ids, out_mask, out_tt):
    B, L = input_ids.shape
    _expect("pair_expand", *((t, torch.int64, (B * N * (N - 1), Lp)) for t in (out_ids, out_mask, out_tt)))
    if tuple(starts.shape) != (B, N) or tuple(lens.shape) != (B, N):
        raise ValueError("pair_expand: starts/lens shapes")
    _call("mmseq_pair_expand", B, L, N, Lp, _p(input_ids), _p(starts), _p(lens), pad_id,
          int(second_type), _p(out_ids), _p(out_mask), _p(out_tt))


def image_resize_normalize(pixels, table, heights, max_h, max_w, out, mean, std):
    """pixels uint8 (device, packed HWC images), table int64 [n][4] (device), heights: host
    int list (workspace sizing), out f32 [n][3][oh][ow] (device)."""
    n, _, oh, ow = out.shape
    if pixels.dtype != torch.uint8 or table.dtype != torch.int64 or tuple(table.shape) != (n, 4):
        raise ValueError("image_resize: pixels uint8, table int64 [n][4]")
    if out.dtype != torch.float32 or not out.is_contiguous() or out.shape[1] != 3:
        raise ValueError("image_resize: out must be contiguous f32 [n][3][oh][ow]")
    hs = (ctypes.c_int32 * max(n, 1))(*[int(h) for h in heights])
    wsb = lib().mmseq_image_resize_workspace(n, ctypes.cast(hs, _vp), ow)
    ws = torch.empty(max(1, wsb // 4), dtype=torch.float32, device=out.device)
    m = (ctypes.c_float * 3)(*[float(x) for x in mean])
    s = (ctypes.c_float * 3)(*[float(x) for x in std])
    _call("mmseq_image_resize_normalize", n, _p(pixels), _p(table), max_h, max_w, oh, ow,
          ctypes.cast(m, _vp), ctypes.cast(s, _vp), _p(ws), ws.numel() * 4, _p(out))


def lstm_cell_fwd(gx, gh, c, h_out, c_out, act):
    """gx [B][>=4H] rows (stride gx.stride(0)), gh [B][4H], c [B][H] f32."""
    B, H = c.shape
    f32 = torch.float32
    if gx.dtype != f32 or gx.stride(-1) != 1 or gx.shape[-1] < 4 * H:
        raise ValueError("lstm_cell_fwd: gx must be f32 [B][>= 4H] with unit inner stride")
    _expect("lstm_cell_fwd", (gh, f32, (B, 4 * H)), (c, f32, (B, H)), (h_out, f32, B * H),
            (c_out, f32, B * H), (act, f32, 4 * B * H))
    _call("mmseq_lstm_cell_fwd", B, H, _p(gx), gx.stride(0), _p(gh), _p(c), _p(h_out), _p(c_out),
          _p(act))


def lstm_cell_bwd(act, c, c_out, dh, dc_next, dgates, dc_prev):
    B, H = c.shape
    _call("mmseq_lstm_cell_bwd", B, H, _p(act), _p(c), _p(c_out), _p(dh), _p(dc_next), _p(dgates),
          _p(dc_prev))


def beam_workspace(B, N, H, W):
    """Bytes of workspace mmseq_beam_search needs; 0 where the shape is unsupported."""
    return int(lib().mmseq_beam_workspace(B, N, H, W))


def _beam_inputs(what, doc, okey, hist, h0, c0, weights, extra):
    """The checks the decoder entries share -> the 14 input pointers in ABI order. `extra`:
    ((tensor, dtype, shape), ...) outputs / index tensors that must be contiguous too."""
    B, N, H = doc.shape
    w_ih, b_ih, w_hh, b_hh, w_q, b_q, w_pw, w_t, b_t = weights
    shapes = ((doc, (B, N, H)), (okey, (B, N, H)), (hist, (B, N, N, H + 2)), (h0, (B, H)),
              (c0, (B, H)), (w_ih, (4 * H, H)), (b_ih, (4 * H,)), (w_hh, (4 * H, H)),
              (b_hh, (4 * H,)), (w_q, (H, H)), (b_q, (H,)), (w_pw, (H, 4 * (H + 2))),
              (w_t, H), (b_t, 1))  # tanh_linear: weight [H] / bias [1] in any shape
    _expect(what, *((t, torch.float32, shp) for t, shp in shapes), *extra)
    return [_p(t) for t, _ in shapes]


def _ws_bytes(workspace):
    _dev(workspace)
    return workspace.numel() * workspace.element_size()


def beam_search(doc, okey, hist, h0, c0, weights, W, order, score, workspace):
    """mmseq_beam_search: doc / okey [B][N][H], hist [B][N][N][H+2], h0 / c0 [B][H] (f32,
    contiguous); weights = (w_ih, b_ih, w_hh, b_hh, w_q, b_q, w_pw, w_t, b_t) in the head store's
    [out][in] layouts; order int64 [B][N], score f32 [B]; workspace: a uint8 / f32 device tensor
    of at least beam_workspace(B, N, H, W) bytes. Returns the status for MMSEQ_EUNSUPPORTED (the
    caller decides what to do instead) and raises on every other failure."""
    B, N, H = doc.shape
    ptrs = _beam_inputs("beam_search", doc, okey, hist, h0, c0, weights,
                        ((order, torch.int64, (B, N)), (score, torch.float32, (B,))))
    return _call("mmseq_beam_search", B, N, H, int(W), *ptrs, _p(order), _p(score), _p(workspace),
                 _ws_bytes(workspace), tail=_status)


def beam_search_nbest(doc, okey, hist, h0, c0, weights, W, orders, scores, count, workspace):
    """mmseq_beam_search_nbest: the inputs and workspace of beam_search; orders int64 [B][W][N],
    scores f32 [B][W], count int32 [B]. Rows count[b] .. W-1 are not written. Returns the status
    for MMSEQ_EUNSUPPORTED and raises on every other failure."""
    B, N, H = doc.shape
    W = int(W)
    ptrs = _beam_inputs("beam_search_nbest", doc, okey, hist, h0, c0, weights,
                        ((orders, torch.int64, (B, W, N)), (scores, torch.float32, (B, W)),
                         (count, torch.int32, (B,))))
    return _call("mmseq_beam_search_nbest", B, N, H, W, *ptrs, _p(orders), _p(scores), _p(count),
                 _p(workspace), _ws_bytes(workspace), tail=_status)


def order_score_workspace(B, N, H, K):
    """Bytes of workspace mmseq_order_score needs; 0 where the shape is unsupported."""
    return int(lib().mmseq_order_score_workspace(B, N, H, K))


def _orders_arg(what, orders, B, N):
    """orders int64 [K][N] (one list shared by all stories) or [B][K][N] -> (K, its shape, the
    story stride the ABI takes: 0 for the shared list)."""
    if orders.dim() not in (2, 3):
        raise ValueError(f"{what}: orders must be int64 [K][N] or [B][K][N]")
    K = int(orders.shape[-2])
    return (K, (K, N), 0) if orders.dim() == 2 else (K, (B, K, N), K * N)


def order_score(doc, okey, hist, h0, c0, weights, orders, nll, step_nll, workspace):
    """mmseq_order_score: the inputs of beam_search; orders int64 [K][N] (one list shared by all
    stories) or [B][K][N]; nll f32 [B][K]; step_nll f32 [B][K][N-1] or None; workspace of at
    least order_score_workspace(B, N, H, K) bytes. Returns the status for MMSEQ_EUNSUPPORTED and
    raises on every other failure."""
    B, N, H = doc.shape
    K, oshape, stride = _orders_arg("order_score", orders, B, N)
    extra = [(orders, torch.int64, oshape), (nll, torch.float32, (B, K))]
    if step_nll is not None:
        extra.append((step_nll, torch.float32, (B, K, N - 1)))
    ptrs = _beam_inputs("order_score", doc, okey, hist, h0, c0, weights, extra)
    return _call("mmseq_order_score", B, N, H, K, *ptrs, _p(orders), stride, _p(nll), _p(step_nll),
                 _p(workspace), _ws_bytes(workspace), tail=_status)


def order_score_bwd_workspace(B, N, H, K):
    """Bytes of workspace mmseq_order_score_bwd needs; 0 where the shape is unsupported."""
    return int(lib().mmseq_order_score_bwd_workspace(B, N, H, K))


def order_score_bwd(doc, okey, hist, h0, c0, weights, weights_t, orders, dnll, dins, dweights,
                    workspace):
    """mmseq_order_score_bwd: the inputs of order_score; weights_t = (wt_ih, wt_hh, wt_q, wt_pw),
    the [in][out] copies; dnll f32 [B][K]; dins = (ddoc, dokey, dhist, dh0, dc0), WRITTEN;
    dweights = the nine weight gradients in the order of `weights`, ACCUMULATED (+=); workspace of
    at least order_score_bwd_workspace(B, N, H, K) bytes. Returns the status for
    MMSEQ_EUNSUPPORTED and raises on every other failure."""
    B, N, H = doc.shape
    K, oshape, stride = _orders_arg("order_score_bwd", orders, B, N)
    if len(weights_t) != 4 or len(dins) != 5 or len(dweights) != 9:
        raise ValueError("order_score_bwd: 4 transposed weights, 5 input and 9 weight gradients "
                         "expected")
    f32 = torch.float32
    extra = [(orders, torch.int64, oshape), (dnll, f32, (B, K))]
    extra += zip(dins, [f32] * 5, ((B, N, H), (B, N, H), (B, N, N, H + 2), (B, H), (B, H)))
    extra += zip(weights_t, [f32] * 4, ((H, 4 * H), (H, 4 * H), (H, H), (4 * (H + 2), H)))
    extra += [(g, f32, tuple(w.shape)) for g, w in zip(dweights[:7], weights[:7])]
    extra += zip(dweights[7:], [f32] * 2, (H, 1))  # tanh_linear gradients, as w_t / b_t
    ptrs = _beam_inputs("order_score_bwd", doc, okey, hist, h0, c0, weights, extra)
    return _call("mmseq_order_score_bwd", B, N, H, K, *ptrs, *[_p(t) for t in weights_t],
                 _p(orders), stride, _p(dnll), *[_p(t) for t in dins], *[_p(t) for t in dweights],
                 _p(workspace), _ws_bytes(workspace), tail=_status)


def order_sample_workspace(B, N, H, S):
    """Bytes of workspace mmseq_order_sample needs; 0 where the shape is unsupported."""
    return int(lib().mmseq_order_sample_workspace(B, N, H, S))


def order_sample(doc, okey, hist, h0, c0, weights, seed, stream_id, story0, sample0, orders, nll,
                 u, step_nlp, workspace):
    """mmseq_order_sample: the inputs of beam_search; orders int64 [B][S][N], nll f32 [B][S], u f32
    [B][S][N-1] or None, step_nlp f32 [B][S][N-1][N] or None; workspace of at least
    order_sample_workspace(B, N, H, S) bytes. Returns the status for MMSEQ_EUNSUPPORTED and
    raises on every other failure."""
    B, N, H = doc.shape
    if orders.dim() != 3:
        raise ValueError("order_sample: orders must be int64 [B][S][N]")
    S = int(orders.shape[1])
    extra = [(orders, torch.int64, (B, S, N)), (nll, torch.float32, (B, S))]
    if u is not None:
        extra.append((u, torch.float32, (B, S, N - 1)))
    if step_nlp is not None:
        extra.append((step_nlp, torch.float32, (B, S, N - 1, N)))
    ptrs = _beam_inputs("order_sample", doc, okey, hist, h0, c0, weights, extra)
    return _call("mmseq_order_sample", B, N, H, S, *ptrs, int(seed) & 0xFFFFFFFFFFFFFFFF,
                 int(stream_id) & 0xFFFFFFFF, int(story0), int(sample0), _p(orders), _p(nll), _p(u),
                 _p(step_nlp), _p(workspace), _ws_bytes(workspace), tail=_status)


def order_tree_workspace(B, N, H, rows):
    """Bytes of workspace mmseq_order_tree needs at a chunk cap of `rows` slot rows; 0 where the
    shape is unsupported or rows < B * N."""
    return int(lib().mmseq_order_tree_workspace(B, N, H, int(rows)))


def order_tree(doc, okey, hist, h0, c0, weights, rows, nll, orders, workspace):
    """mmseq_order_tree: the inputs of beam_search; rows >= B * N, the cap on the slot rows of one
    chunk; nll f32 [B][N!]; orders int64 [N!][N] or None; workspace of at least
    order_tree_workspace(B, N, H, rows) bytes. Returns the status for MMSEQ_EUNSUPPORTED and
    raises on every other failure."""
    B, N, H = doc.shape
    K = math.factorial(N)
    extra = [(nll, torch.float32, (B, K))]
    if orders is not None:
        extra.append((orders, torch.int64, (K, N)))
    ptrs = _beam_inputs("order_tree", doc, okey, hist, h0, c0, weights, extra)
    return _call("mmseq_order_tree", B, N, H, *ptrs, int(rows), _p(nll), _p(orders), _p(workspace),
                 _ws_bytes(workspace), tail=_status)


POSTERIOR_MODES = {"weights": 0, "uniform": 1}
# name -> (dtype, trailing shape in units of N) of mmseq_order_posterior's outputs, in ABI order
POSTERIOR_OUTPUTS = (("logz", torch.float32, 0), ("position", torch.float32, 2),
                     ("before", torch.float32, 2), ("entropy", torch.float32, 0),
                     ("map_index", torch.int32, 0), ("map_prob", torch.float32, 0),
                     ("mbr_acc_index", torch.int32, 0), ("mbr_tau_index", torch.int32, 0),
                     ("exp_acc", torch.float32, 0), ("exp_tau", torch.float32, 0))


def order_posterior(orders, nll, mode, out):
    """mmseq_order_posterior: orders int64 [K][N] or [B][K][N], nll f32 [B][K], mode 0 / 1, out:
    dict name -> contiguous device tensor for every entry of POSTERIOR_OUTPUTS ([B], or [B][N][N]
    for the two matrices). Returns the status for MMSEQ_EUNSUPPORTED and raises on every other
    failure."""
    if nll.dim() != 2 or orders.dim() not in (2, 3):
        raise ValueError("order_posterior: nll must be [B][K], orders [K][N] or [B][K][N]")
    B, K = nll.shape
    N = int(orders.shape[-1])
    shared = orders.dim() == 2
    _expect("order_posterior", (orders, torch.int64, (K, N) if shared else (B, K, N)),
            (nll, torch.float32, (B, K)),
            *((out[name], dtype, (B,) + (N,) * nn) for name, dtype, nn in POSTERIOR_OUTPUTS))
    return _call("mmseq_order_posterior", B, N, K, int(mode), _p(orders), 0 if shared else K * N,
                 _p(nll), *(_p(out[name]) for name, _, _ in POSTERIOR_OUTPUTS), tail=_status)


# name -> (dtype, trailing shape in units of N) of mmseq_pairwise_order's outputs, in ABI order
PAIRWISE_OUTPUTS = (("order", torch.int64, 1), ("pnll", torch.float32, 0),
                    ("margin", torch.float32, 0), ("logz", torch.float32, 0),
                    ("position", torch.float32, 2), ("before", torch.float32, 2),
                    ("entropy", torch.float32, 0))


def pairwise_order_workspace(B, N):
    """Bytes of workspace mmseq_pairwise_order needs; 0 where the shape is unsupported."""
    return int(lib().mmseq_pairwise_order_workspace(B, N))


def pairwise_order(w, out, workspace):
    """mmseq_pairwise_order: w f32 [B][N][N]; out: dict name -> contiguous device tensor for every
    entry of PAIRWISE_OUTPUTS ([B], [B][N] for the order, [B][N][N] for the two matrices);
    workspace of at least pairwise_order_workspace(B, N) bytes. Returns the status for
    MMSEQ_EUNSUPPORTED and raises on every other failure."""
    if w.dim() != 3 or w.shape[1] != w.shape[2]:
        raise ValueError(f"pairwise_order: w must be [B][N][N], got {tuple(w.shape)}")
    B, N = int(w.shape[0]), int(w.shape[1])
    _expect("pairwise_order", (w, torch.float32, (B, N, N)),
            *((out[name], dtype, (B,) + (N,) * nn) for name, dtype, nn in PAIRWISE_OUTPUTS))
    return _call("mmseq_pairwise_order", B, N, _p(w),
                 *(_p(out[name]) for name, _, _ in PAIRWISE_OUTPUTS), _p(workspace),
                 _ws_bytes(workspace), tail=_status)


def pairwise_score(w, orders, pnll):
    """mmseq_pairwise_score: w f32 [B][N][N], orders int64 [K][N] or [B][K][N], pnll f32 [B][K].
    Returns the status for MMSEQ_EUNSUPPORTED and raises on every other failure."""
    if w.dim() != 3 or w.shape[1] != w.shape[2] or orders.dim() not in (2, 3):
        raise ValueError("pairwise_score: w must be [B][N][N], orders [K][N] or [B][K][N]")
    B, N = int(w.shape[0]), int(w.shape[1])
    K, oshape, stride = _orders_arg("pairwise_score", orders, B, N)
    _expect("pairwise_score", (w, torch.float32, (B, N, N)), (orders, torch.int64, oshape),
            (pnll, torch.float32, (B, K)))
    return _call("mmseq_pairwise_score", B, N, K, _p(w), _p(orders), stride, _p(pnll), tail=_status)


def _gather_args(what, big, small, src, keep):
    """big [R_in][cols] or [P][rpb][cols] (R_in = P * rpb, any row / batch strides: mmseq_rows) and
    small [R_out][cols] (any row stride): same dtype, unit inner stride; src int32 [R_out], keep
    uint8 [R_out] or None, contiguous. -> (R_out, R_in, cols, rows of big, rows of small)."""
    _dev(big, small, src, keep)
    if big.dim() not in (2, 3) or small.dim() != 2 or big.shape[-1] != small.shape[1] or \
            big.dtype != small.dtype:
        raise ValueError(f"{what}: [R_in][cols] (or [P][rpb][cols]) and [R_out][cols] of one dtype "
                         "expected")
    for t in (big, small):
        if t.shape[-1] > 1 and t.stride(-1) != 1:
            raise ValueError(f"{what}: unit inner stride expected")
    R_out = small.shape[0]
    _expect(what, (src, torch.int32, R_out), *([(keep, torch.uint8, R_out)] if keep is not None else []))
    if big.dim() == 3:
        bl = rows(big.stride(1), big.stride(0), max(big.shape[1], 1))
        R_in = big.shape[0] * big.shape[1]
    else:
        bl, R_in = rows(big.stride(0)), big.shape[0]
    return R_out, R_in, big.shape[-1], bl, rows(small.stride(0))


def rows_gather_fwd(x, src, keep, out):
    """out[r] = keep[r] ? x[src[r]] : 0 (mmseq_rows_gather_fwd); x [R_in][cols] or [P][rpb][cols],
    out [R_out][cols]. src entries must be unique and in [0, R_in). Raises Unsupported unless
    cols % 8 == 0 and the rows are 16-byte aligned."""
    R_out, R_in, cols, xl, ol = _gather_args("rows_gather_fwd", x, out, src, keep)
    _call("mmseq_rows_gather_fwd", R_out, R_in, cols, _p(x), xl, _p(src), _p(keep), _p(out), ol,
          dt(x), tail=_check_shape)


def rows_gather_bwd(dout, src, keep, din):
    """din = 0, then din[src[r]] = keep[r] ? dout[r] : 0 (mmseq_rows_gather_bwd); din shaped as the
    forward's x, dout as its out."""
    R_out, R_in, cols, dl, ol = _gather_args("rows_gather_bwd", din, dout, src, keep)
    _call("mmseq_rows_gather_bwd", R_out, R_in, cols, _p(dout), ol, _p(src), _p(keep), _p(din), dl,
          dt(din), tail=_check_shape)


def _xent_args(what, logits, V, labels, lse, stats):
    """logits: contiguous [M][ld], the first V columns data (the kernels touch whole 16-byte chunks
    of a row and the backward writes all ld columns, so ld is the tensor's width, not a stride);
    labels int64 [M], lse f32 [M], stats f32 [2] (optional for xent_eval)."""
    _dev(logits)
    if logits.dim() != 2 or not logits.is_contiguous():
        raise ValueError(f"{what}: contiguous logits [M][ld] expected")
    M, ld = logits.shape
    if not 1 <= V <= ld:
        raise ValueError(f"{what}: V = {V} outside the {ld} columns of logits")
    _expect(what, (labels, torch.int64, M), (lse, torch.float32, M),
            *([] if stats is None and what == "xent_eval" else [(stats, torch.float32, 2)]))
    return M, ld


def xent_fwd(logits, V, labels, ignore_index, lse, loss_row, stats):
    """Cross-entropy forward (mmseq_xent_fwd): lse / loss_row f32 [M], stats f32 [2] = (mean loss
    over the rows with label != ignore_index, their count)."""
    M, ld = _xent_args("xent_fwd", logits, V, labels, lse, stats)
    _expect("xent_fwd", (loss_row, torch.float32, M))
    _call("mmseq_xent_fwd", M, V, _p(logits), ld, _p(labels), ignore_index, _p(lse), _p(loss_row),
          _p(stats), dt(logits), tail=_check_shape)


def xent_bwd(logits, V, labels, ignore_index, lse, stats, g=None):
    """logits <- dlogits in place, zeros in ignored rows and in the columns >= V (mmseq_xent_bwd);
    g: the upstream gradient, one f32 on the device, or None for 1."""
    M, ld = _xent_args("xent_bwd", logits, V, labels, lse, stats)
    if g is not None:
        _expect("xent_bwd", (g, torch.float32, 1))
    _call("mmseq_xent_bwd", M, V, _p(logits), ld, _p(labels), ignore_index, _p(lse), _p(stats), _p(g),
          dt(logits), tail=_check_shape)


def xent_eval(logits, V, labels, ignore_index, k, lse, loss_row, rank, topk_idx=None,
              topk_logit=None, totals=None, stats=None):
    """The forward's pass with the evaluation quantities (mmseq_xent_eval): lse / loss_row f32 [M]
    (the bits xent_fwd writes), rank int32 [M], topk_idx int32 [M][k] and topk_logit f32 [M][k]
    (both may be None with k == 0) in the order (value descending, column ascending), totals
    f64 [4] or None, accumulated. `stats` f32 [2] or None: (mean loss over the kept rows, their
    count) with xent_fwd's bits, reduced from loss_row (mmseq_xent_mean)."""
    M, ld = _xent_args("xent_eval", logits, V, labels, lse, stats)
    k = int(k)
    if not 0 <= k <= XENT_EVAL_MAX_K:
        raise ValueError(f"xent_eval: k = {k} outside [0, {XENT_EVAL_MAX_K}]")
    checks = [(loss_row, torch.float32, M), (rank, torch.int32, M)]
    checks += [(t, d, (M, k)) for t, d in ((topk_idx, torch.int32), (topk_logit, torch.float32))
               if not (t is None and k == 0)]
    if totals is not None:
        checks.append((totals, torch.float64, 4))
    _expect("xent_eval", *checks)
    _call("mmseq_xent_eval", M, V, _p(logits), ld, _p(labels), ignore_index, k, _p(lse),
          _p(loss_row), _p(rank), _p(topk_idx), _p(topk_logit), _p(totals), dt(logits),
          tail=_check_shape)
    if stats is not None:
        _call("mmseq_xent_mean", M, _p(loss_row), _p(labels), ignore_index, _p(stats))


def mlm_mask(input_ids, labels, pad_id, cls_id, mask_id, vocab, ignore_index, p, seed, stream_id=0):
    """mask_tokens_sentence on the device (mmseq_mlm_mask): input_ids int64 [B][L] masked in place,
    labels int64 [B][L] written; a pure function of (seed, stream_id, element index)."""
    if not torch.is_tensor(input_ids) or input_ids.dim() != 2:
        raise ValueError("mlm_mask: input_ids must be a tensor [B][L]")
    B, L = input_ids.shape
    _expect("mlm_mask", (input_ids, torch.int64, (B, L)), (labels, torch.int64, (B, L)))
    _call("mmseq_mlm_mask", B, L, _p(input_ids), _p(labels), pad_id, cls_id, mask_id, vocab,
          ignore_index, float(p), seed & 0xFFFFFFFFFFFFFFFF, stream_id & 0xFFFFFFFF)


def subsample_text(input_ids, attention_mask, token_type_ids, labels, sub_idx, n_steps, cls_id,
                   pad_id, ignore_index, out_ids, out_mask, out_tt, out_labels, status):
    """The text of the sub-sampled steps (mmseq_subsample_text): inputs int64 [B][L]
    (token_type_ids / labels may be None, with their outputs), sub_idx int64 [B][n_sub], outputs
    int64 [B][L // n_steps * n_sub]; status int32, zeroed by the caller: status[0] += bad stories."""
    if not torch.is_tensor(input_ids) or input_ids.dim() != 2 or \
            not torch.is_tensor(sub_idx) or sub_idx.dim() != 2:
        raise ValueError("subsample_text: input_ids [B][L] and sub_idx [B][n_sub] expected")
    B, L = input_ids.shape
    n_sub = sub_idx.shape[1]
    pad = L // n_steps * n_sub
    i64 = torch.int64
    checks = [(sub_idx, i64, (B, n_sub))]
    for t, o, optional in ((input_ids, out_ids, False), (attention_mask, out_mask, False),
                           (token_type_ids, out_tt, True), (labels, out_labels, True)):
        if not (optional and t is None and o is None):
            checks += [(t, i64, (B, L)), (o, i64, (B, pad))]
    _expect("subsample_text", *checks)
    if not torch.is_tensor(status) or status.dtype != torch.int32 or status.numel() < 1:
        raise ValueError("subsample_text: status must be int32 on the device")
    _dev(status)
    _call("mmseq_subsample_text", B, L, n_steps, n_sub, _p(input_ids), _p(attention_mask),
          _p(token_type_ids), _p(labels), _p(sub_idx), cls_id, pad_id, ignore_index, _p(out_ids),
          _p(out_mask), _p(out_tt), _p(out_labels), _p(status))


def rows_compact(labels, ignore_index, src, out_labels, count):
    """src int32 [R] / out_labels int64 [R]: their first count[0] entries = the rows r, ascending,
    with labels[r] != ignore_index, and those labels (mmseq_rows_compact); labels int64 [R], count
    int32 [1], all on the device. Nothing at or beyond count[0] is written."""
    if not torch.is_tensor(labels) or labels.dim() != 1:
        raise ValueError("rows_compact: labels must be a tensor [R]")
    R = labels.numel()
    _expect("rows_compact", (labels, torch.int64, (R,)), (out_labels, torch.int64, (R,)),
            (src, torch.int32, R), (count, torch.int32, 1))
    if R >= 1 << 31:
        raise ValueError("rows_compact: R must be below 2^31")
    _call("mmseq_rows_compact", R, _p(labels), ignore_index, _p(src), _p(out_labels), _p(count))


def quant_mxfp8(x, out=None):
    """x [rows][K] bf16 / f32 (K % 32 == 0, unit inner stride) -> MXFP8 (mmseq_quant_mxfp8)."""
    rows, K = x.shape
    if x.stride(-1) != 1 or K % 32:
        raise ValueError("quant_mxfp8: [rows][K] with unit inner stride and K % 32 == 0")
    if out is None:
        out = MXFP8.alloc(rows, K, x.device, zero_scales=False)
    _call("mmseq_quant_mxfp8", rows, K, _p(x), x.stride(0), dt(x), _p(out.q), out.q.stride(0),
          _p(out.scales))
    return out


def attn_fwd_mxfp8(P, T, heads, qkv, ld_qkv, q_off, k_off, v_off, key_bias, scale, lse):
    """Eval attention forward whose output is MX-fp8 (mmseq_attn_fwd_mxfp8): MXFP8 [P*T][heads*64],
    the output projection's fp8 operand; padding-row scales zeroed here."""
    o = MXFP8.alloc(P * T, heads * 64, qkv.device, zero_scales=True)
    _call("mmseq_attn_fwd_mxfp8", P, T, heads, _p(qkv), ld_qkv, q_off, k_off, v_off, _p(key_bias),
          scale, _p(lse), _p(o.q), o.q.stride(0), _p(o.scales))
    return o


def attn_bwd_mxfp8(P, T, heads, qkv, key_bias, scale, out, dout, lse, delta, dqkv, drop=None,
                   keep_bits=None):
    """attn_bwd (bf16 fast kernels, packed Q|K|V) that also returns dQ|dK|dV in MX-fp8
    (mmseq_attn_bwd_mxfp8): the QKV dgrad GEMM's operand in config 5's fp8 dgrad; padding-row
    scales zeroed here."""
    o = MXFP8.alloc(P * T, 3 * heads * 64, qkv.device, zero_scales=True)
    _call("mmseq_attn_bwd_mxfp8", P, T, heads, _p(qkv), qkv.stride(0), _p(key_bias), scale, _p(out),
          out.stride(0), _p(dout), dout.stride(0), _p(lse), _p(delta), _p(dqkv), dqkv.stride(0),
          _d(drop), _p(keep_bits), _p(o.q), o.q.stride(0), _p(o.scales))
    return o


def attn_fwd_mxfp8_dual(P, T, heads, qkv, ld_qkv, q_off, k_off, v_off, key_bias, scale, out, ld_out,
                        lse, drop=None, keep_bits=None):
    """Training attention forward with the bf16 output `out` (None: MX-fp8 only) AND its MX-fp8
    copy (the fp8 output projection's operand), dropout / keep bits as attn_fwd
    (mmseq_attn_fwd_mxfp8_dual) -> MXFP8 [P*T][heads*64]; padding-row scales zeroed here."""
    _dev(out)
    o = MXFP8.alloc(P * T, heads * 64, qkv.device, zero_scales=True)
    _call("mmseq_attn_fwd_mxfp8_dual", P, T, heads, _p(qkv), ld_qkv, q_off, k_off, v_off,
          _p(key_bias), scale, _p(out), ld_out, _p(lse), _d(drop), _p(keep_bits), _p(o.q),
          o.q.stride(0), _p(o.scales))
    return o


def gemm_mxfp8_ex(a, b, c=None, bias=None, act=0, aux=None, resid=None, drop=None, q8=False,
                  dact=None):
    """Training fp8 GEMM (mmseq_gemm_mxfp8_ex): c (bf16) = dropout(act(a @ b^T + bias)) + resid,
    aux = pre-activation; with q8=True also returns the MX-fp8 copy of the output (FC1: no resid /
    drop); with dact the dgrad form c = (a @ b^T) * act'(dact). Returns the MXFP8 output (q8) or
    None."""
    if a.K != b.K:
        raise ValueError("gemm_mxfp8_ex: K mismatch")
    rows, Nn = a.rows, b.rows
    for t in (c, aux, resid, dact):
        if t is not None and (t.dtype != torch.bfloat16 or tuple(t.shape) != (rows, Nn)):
            raise ValueError("gemm_mxfp8_ex: bf16 [rows][N] outputs / residual")
    o = MXFP8.alloc(rows, Nn, a.q.device, zero_scales=False) if q8 else None
    q, sc = (o.q, o.scales) if q8 else (None, None)
    ld = c.stride(0) if c is not None else (aux.stride(0) if aux is not None else Nn)
    _call("mmseq_gemm_mxfp8_ex", rows, Nn, a.K, _p(a.q), a.q.stride(0), _p(a.scales), _p(b.q),
          b.q.stride(0), _p(b.scales), _p(c), ld, _p(bias), act, _p(aux), _p(dact), _p(resid),
          resid.stride(0) if resid is not None else 0, _d(drop), _p(q),
          q.stride(0) if q8 else 0, _p(sc))
    return o


def gemm_mxfp8(a, b, c, bias=None, act=0, resid=None, alpha=1.0):
    """c[m][n] (bf16) = act(alpha * a @ b^T + bias) + resid, a / b MXFP8 operands."""
    if a.K != b.K or tuple(c.shape) != (a.rows, b.rows) or c.dtype != torch.bfloat16:
        raise ValueError("gemm_mxfp8: shapes / dtype")
    if resid is not None and (resid.dtype != torch.bfloat16 or tuple(resid.shape) != tuple(c.shape)):
        raise ValueError("gemm_mxfp8: resid")
    _call("mmseq_gemm_mxfp8", a.rows, b.rows, a.K, _p(a.q), a.q.stride(0), _p(a.scales), _p(b.q),
          b.q.stride(0), _p(b.scales), _p(c), c.stride(0), _p(bias), act, _p(resid),
          resid.stride(0) if resid is not None else 0, alpha)


def gemm_mxfp8_out(x, W, bias=None, act=0):
    """MXFP8 of bf16(act(x @ W^T + bias)) (x [rows][K], W [N][K] bf16) straight from the GEMM
    epilogue (mmseq_gemm_mxfp8_out): the consumer GEMM's A operand without a quantisation pass."""
    rows, K = x.shape
    Nn = W.shape[0]
    if x.dtype != torch.bfloat16 or W.dtype != torch.bfloat16 or W.shape[1] != K:
        raise ValueError("gemm_mxfp8_out: bf16 x [rows][K], W [N][K]")
    o = MXFP8.alloc(rows, Nn, x.device, zero_scales=False)
    _call("mmseq_gemm_mxfp8_out", rows, Nn, K, _p(x), x.stride(0), _p(W), W.stride(0), _p(bias), act,
          _p(o.q), o.q.stride(0), _p(o.scales))
    return o


def gemm_mxfp8_q8(a, b, bias=None, act=0):
    """MXFP8 of bf16(act(a @ b^T + bias)) for MXFP8 operands a [rows][K], b [N][K]
    (mmseq_gemm_mxfp8_q8): an fp8 GEMM whose output is the next fp8 GEMM's A operand."""
    if a.K != b.K:
        raise ValueError("gemm_mxfp8_q8: K mismatch")
    o = MXFP8.alloc(a.rows, b.rows, a.q.device, zero_scales=False)
    _call("mmseq_gemm_mxfp8_q8", a.rows, b.rows, a.K, _p(a.q), a.q.stride(0), _p(a.scales), _p(b.q),
          b.q.stride(0), _p(b.scales), _p(bias), act, _p(o.q), o.q.stride(0), _p(o.scales))
    return o


# -- RN50 (csrc/resnet.hip) ----------------------------------------------------------------------
def conv_im2col(x, ks, stride, pad, Kp, cols):
    U, H, W, C = x.shape
    _call("mmseq_conv_im2col", U, H, W, C, ks, stride, pad, Kp, _p(x), _p(cols), dt(x))


def conv_col2im(dcols, U, H, W, C, ks, stride, pad, Kp, dx):
    _call("mmseq_conv_col2im", U, H, W, C, ks, stride, pad, Kp, _p(dcols), _p(dx), dt(dx))


def _bn_ws(rows, C, device):
    return torch.empty(max(1, lib().mmseq_bn_workspace(rows, C) // 4), dtype=torch.float32,
                       device=device)


def bn_fwd(x, gamma, beta, resid, relu, train, eps, momentum, n_ref, mean, rstd, run_mean,
           run_var, y):
    C = x.shape[-1]
    rows = x.numel() // C
    ws = _bn_ws(rows, C, x.device)
    _call("mmseq_bn_fwd", rows, C, _p(x), _p(gamma), _p(beta), _p(resid), int(relu), int(train), eps,
          momentum, float(n_ref), _p(mean), _p(rstd), _p(run_mean), _p(run_var), _p(y), _p(ws),
          ws.numel() * 4, dt(x))


def bn_bwd(dy, y, x, mean, rstd, gamma, train, dgamma, dbeta, dx, dres=None):
    C = x.shape[-1]
    rows = x.numel() // C
    ws = _bn_ws(rows, C, x.device)
    _call("mmseq_bn_bwd", rows, C, _p(dy), _p(y), _p(x), _p(mean), _p(rstd), _p(gamma), int(train),
          _p(dgamma), _p(dbeta), _p(dx), _p(dres), _p(ws), ws.numel() * 4, dt(x))


def avgpool2(x, y, backward=False):
    """forward: x [U][H][W][C] -> y [U][H/2][W/2][C]; backward: x = dy, y = dx [U][H][W][C]."""
    U, H, W, C = (y.shape if backward else x.shape)
    _call("mmseq_avgpool2", U, H, W, C, _p(x), _p(y), int(backward), dt(x))


def attnpool_gather(feats, pairimg, pos, x):
    P, T2, C = x.shape
    S = (T2 - 1) // 2
    _call("mmseq_attnpool_gather", P, S, C, _p(feats), _p(pairimg), _p(pos), _p(x), dt(x))


def attnpool_gather_bwd(dx, N, rolepairs, dfeats):
    U, S, C = dfeats.shape
    _call("mmseq_attnpool_gather_bwd", U, N, S, C, N * (N - 1), _p(dx), _p(rolepairs), _p(dfeats),
          dt(dfeats))


def attnpool_out(a, G, xpos, ypos, ttype, y):
    rows, Ch = a.shape
    T2 = 2 * G * G + 1
    _call("mmseq_attnpool_out", rows, T2, Ch, G, _p(a), _p(xpos), _p(ypos), _p(ttype), _p(y), dt(a))


def attnpool_out_bwd(dy, P, T2, Ch, da, token_colsum):
    _call("mmseq_attnpool_out_bwd", P, T2, Ch, _p(dy), _p(da), _p(token_colsum), dt(dy))
