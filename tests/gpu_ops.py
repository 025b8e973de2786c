"""Thin test-side callers of the per-block C-ABI entry points (tests only)."""
import ctypes as C

import torch

from l3ac_amd import _capi


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def to_frames(x_bct: torch.Tensor) -> torch.Tensor:
    """reference layout (B, C, T) -> frame-major (B, T, C) contiguous on the GPU."""
    return x_bct.permute(0, 2, 1).contiguous().cuda()


def from_frames(y_btc: torch.Tensor) -> torch.Tensor:
    return y_btc.permute(0, 2, 1).contiguous().cpu()


def op_block(ctx, fn_name, block, x_btc, out_shape, out=None):
    """out: the caller's output of out_shape (contiguous) instead of a new tensor; the same in every helper below that takes it."""
    y = torch.empty(out_shape, dtype=torch.float32, device=x_btc.device) if out is None else _out(out, out_shape, torch.float32)
    b, frames = x_btc.shape[0], x_btc.shape[1]
    fn = getattr(ctx.lib, fn_name)
    _capi.check(fn(ctx.handle, block.encode(), x_btc.data_ptr(), b, frames, y.data_ptr(), _stream(x_btc.device)))
    torch.cuda.synchronize()
    return y


def _out(out, shape, dtype):
    assert tuple(out.shape) == tuple(shape) and out.dtype == dtype and out.is_contiguous(), f"out is {tuple(out.shape)} {out.dtype}, wanted {tuple(shape)} {dtype}"
    return out


def op_block2(ctx, fn_name, block_a, block_b, x_btc, out_shape, out=None):
    y = torch.empty(out_shape, dtype=torch.float32, device=x_btc.device) if out is None else out
    b, frames = x_btc.shape[0], x_btc.shape[1]
    fn = getattr(ctx.lib, fn_name)
    _capi.check(fn(ctx.handle, block_a.encode(), block_b.encode(), x_btc.data_ptr(), b, frames, y.data_ptr(), _stream(x_btc.device)))
    torch.cuda.synchronize()
    return y


def op_plain(ctx, fn_name, x, d1, d2, out_shape, out_dtype=torch.float32, out=None):
    y = torch.empty(out_shape, dtype=out_dtype, device=x.device) if out is None else _out(out, out_shape, out_dtype)
    fn = getattr(ctx.lib, fn_name)
    _capi.check(fn(ctx.handle, x.data_ptr(), d1, d2, y.data_ptr(), _stream(x.device)))
    torch.cuda.synchronize()
    return y


def legacy_unit(ctx, unit, x_btc, out=None):
    """l3ac_op_legacy_unit: LegacyUnit `unit` (0, 1, 2 = dilation 1, 3, 9) on x [B][T][C] -> [B][T][C]."""
    y = torch.empty_like(x_btc) if out is None else out
    b, frames = x_btc.shape[0], x_btc.shape[1]
    _capi.check(ctx.lib.l3ac_op_legacy_unit(ctx.handle, unit, x_btc.data_ptr(), b, frames, y.data_ptr(), _stream(x_btc.device)))
    torch.cuda.synchronize()
    return y


def first_block_at(ctx, audio, samples=None, frames=None, out=None):
    """l3ac_op_first_block_at: the stem on audio [B][stride] (GPU), of which each row's first `samples` floats are the clip (default:
    the whole row), -> [B][frames][d0]; frames > samples: the zero right-padding folded into the load."""
    b, stride = audio.shape[0], audio.stride(0) if audio.shape[0] > 1 else audio.shape[1]
    samples = audio.shape[1] if samples is None else samples
    frames = samples if frames is None else frames
    shape = (b, max(frames, 1), ctx.mc.encoder_dims[0])
    y = torch.empty(shape, dtype=torch.float32, device=audio.device) if out is None else _out(out, shape, torch.float32)
    _capi.check(ctx.lib.l3ac_op_first_block_at(ctx.handle, audio.data_ptr(), b, samples, stride, frames, y.data_ptr(), _stream(audio.device)))
    torch.cuda.synchronize()
    return y


def head(ctx, x_btc, out=None):
    """l3ac_op_head: snake -> Conv1d(C -> 1, k7) -> tanh (unless the context's head_pretanh is on), x [B][T][C] -> [B][T]."""
    return op_plain(ctx, "l3ac_op_head", x_btc, x_btc.shape[0], x_btc.shape[1], (x_btc.shape[0], x_btc.shape[1]), out=out)


def fsq_forward(x, levels, w_in, b_in, w_out, b_out, latents_in=None, want_latents=False, out=None):
    """out: (q, indices, level_indices) or, with want_latents, (q, indices, level_indices, latents), the caller's own."""
    lib = _capi.load_library()
    dev = w_out.device
    feat = w_out.shape[0]
    d = len(levels)
    n = (x if x is not None else latents_in).reshape(-1, feat if x is not None else d).shape[0]
    q, idx, li = _fsq_outs(out, n, feat, d, dev)
    lv = (C.c_int32 * d)(*levels)
    if x is not None:
        lat = None
        if want_latents:
            lat = torch.empty((n, d), dtype=torch.float32, device=dev) if out is None else _out(out[3], (n, d), torch.float32)
        if out is None:
            x = x.reshape(n, feat).contiguous()
        else:
            assert tuple(x.shape) == (n, feat) and x.is_contiguous()  # (the caller placed it: no copy)
        xp = x.data_ptr()
    else:
        lat = latents_in.reshape(n, d).contiguous().clone()
        xp = None
    _capi.check(lib.l3ac_fsq_forward(xp, n, feat, lv, d, w_in.data_ptr() if w_in is not None else None,
                                     b_in.data_ptr() if b_in is not None else None, w_out.data_ptr(), b_out.data_ptr(),
                                     q.data_ptr(), idx.data_ptr(), li.data_ptr(), lat.data_ptr() if lat is not None else None,
                                     _stream(dev)))
    torch.cuda.synchronize()
    return q, idx, li, lat


def _fsq_outs(out, n, feat, d, dev):
    if out is None:
        return (torch.empty((n, feat), dtype=torch.float32, device=dev), torch.empty((n,), dtype=torch.int32, device=dev),
                torch.empty((n, d), dtype=torch.float32, device=dev))
    return _out(out[0], (n, feat), torch.float32), _out(out[1], (n,), torch.int32), _out(out[2], (n, d), torch.float32)


def fsq_quantize_act(act, levels, w_out, b_out, out=None):
    """SuperFSQ.quantize_act_value onwards (vq/fsq.py:56-68), from activation values in [0, 1]."""
    lib = _capi.load_library()
    dev = w_out.device
    feat, d = w_out.shape[0], len(levels)
    if out is None:
        act = act.reshape(-1, d).contiguous()
    else:
        assert act.dim() == 2 and act.shape[1] == d and act.is_contiguous()  # (the caller placed it: no copy)
    n = act.shape[0]
    q, idx, li = _fsq_outs(out, n, feat, d, dev)
    _capi.check(lib.l3ac_fsq_quantize_act(act.data_ptr(), n, feat, (C.c_int32 * d)(*levels), d, w_out.data_ptr(), b_out.data_ptr(),
                                          q.data_ptr(), idx.data_ptr(), li.data_ptr(), _stream(dev)))
    torch.cuda.synchronize()
    return q, idx, li


def fsq_decode(indices, levels, w_out, b_out, out=None):
    lib = _capi.load_library()
    dev = w_out.device
    feat = w_out.shape[0]
    if out is None:
        idx = indices.reshape(-1).to(torch.int32).contiguous()
    else:
        assert indices.dim() == 1 and indices.dtype == torch.int32 and indices.is_contiguous()  # (the caller placed it: no copy)
        idx = indices
    n = idx.shape[0]
    q = torch.empty((n, feat), dtype=torch.float32, device=dev) if out is None else _out(out, (n, feat), torch.float32)
    lv = (C.c_int32 * len(levels))(*levels)
    _capi.check(lib.l3ac_fsq_decode(idx.data_ptr(), n, feat, lv, len(levels), w_out.data_ptr(), b_out.data_ptr(),
                                    q.data_ptr(), _stream(dev)))
    torch.cuda.synchronize()
    return q


def vq_argmin(queries, codebook, form=0, info=None, out=None, scratch=None):
    """out: the caller's int32 [n]; scratch: the caller's uint8 buffer of exactly l3ac_vq_argmin_scratch_bytes bytes.  form 1: the direct-form scan where the screened form would run (an argument of l3ac_vq_argmin).  info: dict that receives
    'listed' = how many queries the screened form sent to the full direct-form search (first int32 of its scratch)."""
    lib = _capi.load_library()
    n, dim = queries.shape
    out = torch.empty((n,), dtype=torch.int32, device=queries.device) if out is None else _out(out, (n,), torch.int32)
    nbytes = lib.l3ac_vq_argmin_scratch_bytes(n, codebook.shape[0], form)
    if scratch is None:
        scratch = torch.zeros((max(nbytes, 4),), dtype=torch.uint8, device=queries.device)
    else:
        assert scratch.dtype == torch.uint8 and scratch.numel() == nbytes and scratch.is_contiguous()
    _capi.check(lib.l3ac_vq_argmin(queries.data_ptr(), n, codebook.data_ptr(), codebook.shape[0], dim, out.data_ptr(),
                                   scratch.data_ptr(), nbytes, form, _stream(queries.device)))
    torch.cuda.synchronize()
    if info is not None:
        info["listed"] = int(scratch[:4].view(torch.int32).item()) if (form == 0 and n >= 5120) else None
    return out


def _ld(t, ld, what):
    """The leading dimension a GEMM operand is passed with: `ld` when given (the tensor's own row stride must be it, or it has one
    row), else the row stride."""
    if ld is None:
        return t.stride(0)
    assert t.stride(1) == 1 and ld >= t.shape[1] and (t.shape[0] == 1 or t.stride(0) == ld), f"{what}: strides {t.stride()} against ld {ld}"
    return ld


def _gemm_out(out, m, n, ldc, dev):
    """C [m][n] with row stride ldc: a new tensor (dense unless ldc is given), or the caller's view"""
    if out is None:
        return torch.empty((m, n if ldc is None else ldc), dtype=torch.float32, device=dev)[:, :n]
    assert tuple(out.shape) == (m, n) and out.dtype == torch.float32
    return out


def gemm(a, w, bias, out=None, lda=None, ldc=None):
    """lda / ldc: the row strides of a and of C as the C ABI takes them (default: a's own, and n); out: the caller's C, a view [m][n] of
    row stride ldc."""
    lib = _capi.load_library()
    m, k = a.shape
    n = w.shape[0]
    c = _gemm_out(out, m, n, ldc, a.device)
    _capi.check(lib.l3ac_gemm_f32(a.data_ptr(), _ld(a, lda, "a"), w.data_ptr(), bias.data_ptr() if bias is not None else None,
                                  c.data_ptr(), _ld(c, n if ldc is None else ldc, "c"), m, n, k, _stream(a.device)))
    torch.cuda.synchronize()
    return c


def gemm_split(a, w, bias, w256=None, out=None, lda=None, ldc=None):
    """bf16x3 split-operand GEMM through the C ABI: builds the weight image on the device, then multiplies.  w256: which batch products
    take gemm_split_kernel_w256 (0 / 1 / 2, l3ac_gemm_split_f32_at); None: as a new context's option "gemm_w256" would.  out, lda, ldc: as gemm."""
    lib = _capi.load_library()
    m, k = a.shape
    n = w.shape[0]
    nbytes = lib.l3ac_gemm_split_image_bytes(n, k)
    assert nbytes > 0, f"shape n={n} k={k} is not eligible for the split kernel"
    img = torch.empty((nbytes,), dtype=torch.uint8, device=a.device)
    c = _gemm_out(out, m, n, ldc, a.device)
    _capi.check(lib.l3ac_gemm_split_image(w.data_ptr(), n, k, img.data_ptr(), _stream(a.device)))
    args = (a.data_ptr(), _ld(a, lda, "a"), img.data_ptr(), bias.data_ptr() if bias is not None else None, c.data_ptr(),
            _ld(c, n if ldc is None else ldc, "c"), m, n, k)
    if w256 is None:
        _capi.check(lib.l3ac_gemm_split_f32(*args, _stream(a.device)))
    else:
        _capi.check(lib.l3ac_gemm_split_f32_at(*args, w256, _stream(a.device)))
    torch.cuda.synchronize()
    return c


def snake(x, alpha, mode=0, out=None):
    """l3ac_op_snake: x [rows][c], alpha [c]; mode bit 0 = packed form, bit 1 = sin(x)^2 only."""
    lib = _capi.load_library()
    rows, c = x.shape
    y = torch.empty_like(x) if out is None else _out(out, x.shape, x.dtype)
    _capi.check(lib.l3ac_op_snake(x.data_ptr(), y.data_ptr(), rows, c, alpha.data_ptr(), mode, _stream(x.device)))
    torch.cuda.synchronize()
    return y
