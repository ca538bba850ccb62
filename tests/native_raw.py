"""Direct calls of the C ABI (include/mmseq.h) with every leading dimension, offset and buffer
given by the test: the wrappers of `_native` fix the packed production layouts and allocate
outputs themselves, which is what the layout / guard-band tests must not do."""
from multimodal_sequencing_amd import _native as nat

EINVAL = -1
p = nat._p
d = nat._d
status = nat._raw  # the raw mmseq_status of an entry point (the stream is appended)
call = nat._call  # ... checked: raises NativeError on any failure


def attn_fwd(P, T, heads, qkv, ld_qkv, offs, bias, scale, out, ld_out, lse, dtype, variant,
             drop=None, bits=None):
    call("mmseq_attn_fwd", P, T, heads, p(qkv), ld_qkv, *offs, p(bias), scale, p(out), ld_out,
         p(lse), dtype, d(drop), p(bits), variant)


def attn_bwd(P, T, heads, qkv, ld_qkv, offs, bias, scale, out, ld_out, dout, ld_dout, lse, delta,
             dqkv, ld_dqkv, dtype, variant, drop=None, bits=None, check=True):
    st = status("mmseq_attn_bwd", P, T, heads, p(qkv), ld_qkv, *offs, p(bias), scale, p(out),
                ld_out, p(dout), ld_dout, p(lse), p(delta), p(dqkv), ld_dqkv, dtype, d(drop),
                p(bits), variant)
    if check:
        nat._check(st, "mmseq_attn_bwd")
    return st


def attn_fwd_rows(P, T, Tq, heads, qkv, ld_qkv, offs, bias, scale, out, ld_out, lse, drop=None,
                  bits=None):
    call("mmseq_attn_fwd_rows", P, T, Tq, heads, p(qkv), ld_qkv, *offs, p(bias), scale, p(out),
         ld_out, p(lse), d(drop), p(bits))


def attn_bwd_rows(P, T, Tq, heads, qkv, ld_qkv, offs, bias, scale, out, ld_out, dout, ld_dout,
                  lse, delta, dqkv, ld_dqkv, drop=None, bits=None):
    call("mmseq_attn_bwd_rows", P, T, Tq, heads, p(qkv), ld_qkv, *offs, p(bias), scale, p(out),
         ld_out, p(dout), ld_dout, p(lse), p(delta), p(dqkv), ld_dqkv, d(drop), p(bits))


def attn_fwd_mxfp8(P, T, heads, qkv, ld_qkv, offs, bias, scale, lse, q8, ldq8, q8s):
    call("mmseq_attn_fwd_mxfp8", P, T, heads, p(qkv), ld_qkv, *offs, p(bias), scale, p(lse),
         p(q8), ldq8, p(q8s))


def attn_fwd_mxfp8_dual(P, T, heads, qkv, ld_qkv, offs, bias, scale, out, ld_out, lse, q8, ldq8,
                        q8s, drop=None, bits=None):
    call("mmseq_attn_fwd_mxfp8_dual", P, T, heads, p(qkv), ld_qkv, *offs, p(bias), scale, p(out),
         ld_out, p(lse), d(drop), p(bits), p(q8), ldq8, p(q8s))


def attn_bwd_mxfp8(P, T, heads, qkv, ld_qkv, bias, scale, out, ld_out, dout, ld_dout, lse, delta,
                   dqkv, ld_dqkv, q8, ldq8, q8s, drop=None, bits=None):
    call("mmseq_attn_bwd_mxfp8", P, T, heads, p(qkv), ld_qkv, p(bias), scale, p(out), ld_out,
         p(dout), ld_dout, p(lse), p(delta), p(dqkv), ld_dqkv, d(drop), p(bits), p(q8), ldq8,
         p(q8s))
