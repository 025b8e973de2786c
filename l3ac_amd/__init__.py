"""l3ac_amd — MI355X-native encode -> quantize -> decode path behind L3AC's Python surface.

Drop-in for the reference package on this path (``import l3ac_amd as l3ac``):

    l3ac.list_models()                      reference l3ac/__init__.py:17-18
    codec = l3ac.get_model("1kbps")         reference l3ac/__init__.py:21-25
    codec.config.sample_rate                reference l3ac/__init__.py:54-81
    codec.network.to(device="cuda"); codec.network.eval()
    q_feature, indices = codec.encode_audio(audio)          reference l3ac/__init__.py:108-114
    audio = codec.decode_audio(q_feature)                   reference l3ac/__init__.py:116-121
    audio = codec.decode_audio(indices=indices["indices"])

Audio at another rate (44.1 kHz, 48 kHz, ...) is converted on the GPU, where the reference resamples on the CPU first
(its example.py: librosa.resample):

    y16 = l3ac.resample(audio, 48000, codec.config.sample_rate)      scipy.signal.resample_poly's defaults, HIP kernel
    q_feature, indices = codec.encode_audio(audio, sample_rate=48000)    == encode_audio(resample(audio, 48000, 16000))
    audio = codec.decode_audio(q_feature, sample_rate=44100)             == resample(decode_audio(q_feature), 16000, 44100)

All arithmetic runs in hand-written HIP kernels inside libl3ac_hip.so (include/l3ac_hip.h) on gfx950; torch
supplies device memory and streams only.  There is no CPU path: calling encode/decode with CPU tensors, or
without the built extension, raises.
"""
from __future__ import annotations

import logging
import math
import os
import weakref
from pathlib import Path
from typing import Optional

import torch

from . import _capi
from . import weights as _weights
from ._rows import (check_codec_input, contiguous_rows, decode_rows, encode_rows, int_list, refuse_grn_exact, row_stride, validated, window_args,
                    zero_after as _zero_after)
from .chunking import ChunkData, _chunk_cut, _chunk_groups, _chunk_merge, _group_desc, chunk_plan, plan as _chunk_plan
from .metrics import (DEFAULT_SCALES, _check_params as _check_metric_params, _scales as _metric_scales, log_mel, mel_distance, mel_weights,
                      signal_metrics, stft, stft_basis, stft_frames, stoi, stoi_bands, stoi_basis, stoi_frames)
from .loudness import (_check_rate as _check_loudness_rate, apply_gain, loudness, loudness as _loudness, loudness_blocks, loudness_coeffs, loudness_gain,
                       loudness_range, loudness_range as _loudness_range, normalize_loudness, short_term_loudness, true_peak, true_peak as _true_peak,
                       true_peak_factor)
from .pitch import _check_params as _check_pitch_params, pitch, pitch_frames, pitch_lags, pitch_metrics, pitch_metrics as _pitch_metrics
from .align import align, apply_delay, delay
from .mcd import _check_mfcc_params, _mfcc_hop, dct_table, dtw, mcd, mcd as _mcd, mfcc
from .lpc import (_check_params as _check_lpc_params, lpc, lpc_defaults, lpc_frames, lpc_frames as _lpc_frames, lpc_metrics,
                  lpc_metrics as _lpc_metrics, lpc_window)
from .sdr import correlate, sdr, sdr as _sdr, toeplitz_solve
from .bands import (_check_params as _check_band_params, band_energies, band_metrics, band_metrics as _band_metrics, band_weights, critical_bands,
                    frame_spectrum)
from .coherence import coherence, csii, csii as _csii, sii_bands
from .resampling import _resample_bank, resample, resample_length
from .streaming import StreamDecoder, StreamEncoder, StreamResampler, filter_advance
from .filtering import StreamFilter, butter_sos, highpass, k_weighting_sos, sosfilt, sosfilt_matrix, sosfilt_segment
from .wire import (StreamPacker, StreamUnpacker, bits_per_token, frame_header, pack_advance, pack_indices, packed_bytes, parse_frame,
                   unpack_advance, unpack_indices)
from .config import CONFIG_DIR, L3ACConfig, ModelConfig, list_models, resolve_config_file

__all__ = ["set_gemm_split", "get_gemm_split", "gemm_split_routes", "restore_gemm_split_routes", "list_models", "get_model", "get_model_info", "L3AC", "L3ACConfig", "ModelConfig", "Network",
           "bits_per_token", "pack_indices", "unpack_indices", "ChunkData", "resample", "resample_length", "ragged_lengths", "chunk_plan", "StreamEncoder", "StreamDecoder",
           "StreamResampler", "stream_resampler", "StreamPacker", "StreamUnpacker", "stream_packer", "stream_unpacker", "packed_bytes", "pack_advance",
           "unpack_advance", "frame_header", "parse_frame", "stft", "log_mel", "mel_distance", "signal_metrics", "stft_frames", "stft_basis",
           "mel_weights", "DEFAULT_SCALES", "stoi", "stoi_frames", "stoi_basis", "stoi_bands", "loudness", "loudness_gain", "apply_gain",
           "normalize_loudness", "loudness_coeffs", "loudness_blocks", "pitch", "pitch_metrics", "pitch_frames", "pitch_lags", "delay",
           "apply_delay", "align", "mfcc", "dtw", "mcd", "dct_table", "lpc", "lpc_metrics", "lpc_frames", "lpc_defaults", "lpc_window",
           "sdr", "correlate", "toeplitz_solve", "frame_spectrum", "band_energies", "band_metrics", "band_weights", "critical_bands",
           "coherence", "csii", "sii_bands", "sosfilt", "sosfilt_segment", "sosfilt_matrix", "butter_sos", "k_weighting_sos", "highpass",
           "StreamFilter", "stream_filter", "filter_advance", "true_peak", "true_peak_factor", "short_term_loudness", "loudness_range"]
__version__ = "0.1.0"

log = logging.getLogger("L3AC")

# GEMM route: state of each Network's own HIP context.  The module-level setter below keeps the
# round-1/2 convenience (one call switches every live network and the default of later ones) without any process-wide
# state inside the library.
def _env_atoi_flag(name: str, default: bool) -> bool:
    """The library's own reading of a 0/1 environment switch (`std::atoi(value) != 0`, kernels/gemm_split.hip): leading
    whitespace, an optional sign, then digits; anything else ("off", "") counts as 0."""
    import re
    v = os.environ.get(name)
    if v is None:
        return default
    m = re.match(r"\s*([+-]?\d+)", v)
    return bool(m) and int(m.group(1)) != 0


_default_gemm_split = _env_atoi_flag("L3AC_GEMM_SPLIT", True)
_networks: "weakref.WeakSet[Network]" = weakref.WeakSet()


class Network:
    """Stands where the reference's ``EnCodec`` nn.Module stands (``codec.network``): holds the weights and the
    per-device HIP context.  Callers only move it (``.to`` / ``.cuda``) and switch it to eval mode."""

    def __init__(self, mc: ModelConfig):
        mc.check_supported()
        self.mc = mc
        self.training = True  # nn.Module default; the reference needs .eval() before inference (vq/fsq.py:31)
        # GRN (layers.py:112-115) normalises by g / (g + 1e-8), g = the clip's L2 norm over the whole hidden tensor: exactly 1.0f in
        # fp32 for g >= 0.25, which the kernels assume.  grn_exact = True (set BEFORE .to(device)) is the validation mode: the
        # literal two-pass formula is evaluated (correct for any input) and min_grn_norm() reports the smallest g seen, i.e.
        # whether the fast path would have been exact for the data that went through.
        self.grn_exact = False
        self._gemm_split = _default_gemm_split
        _networks.add(self)
        self._state_dicts = None
        self._folded = None
        self._ctx: Optional[_capi.Context] = None
        self.device = torch.device("cpu")

    # ---- weights ------------------------------------------------------------------------------------
    def load_state_dicts(self, state_dicts) -> "Network":
        _weights.check_state_dicts(state_dicts, self.mc)
        self._state_dicts = state_dicts
        self._folded = _weights.folded_weights(state_dicts)  # weight-norm folded once
        if self._ctx is not None:
            self._drop_ctx()
            self._make_ctx()
        return self

    def load_model(self, model_dir=None, model_path=None) -> "Network":
        """reference xtract/nn/module.py:43-54, but a missing file raises instead of keeping random weights."""
        model_path = Path(model_path) if model_path is not None else Path(model_dir)
        return self.load_state_dicts(_weights.load_state_dicts(model_path, self.mc))

    def state_dicts(self):
        return self._state_dicts

    @property
    def trainable_modules(self):
        return {name: self._state_dicts[name] for name in _weights.MODULE_NAMES} if self._state_dicts else {}

    # ---- nn.Module-like surface -----------------------------------------------------------------------
    def eval(self) -> "Network":
        self.training = False
        return self

    def train(self, mode: bool = True) -> "Network":
        if mode:
            raise NotImplementedError("l3ac_amd implements the inference path only (FSQ noise / drop-path are training-side)")
        return self.eval()

    def to(self, device=None, dtype=None, **_ignored) -> "Network":
        if dtype is not None and dtype != torch.float32:
            raise NotImplementedError("the path computes in fp32, like the reference")
        if device is None:
            return self
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if device != self.device:
            self._drop_ctx()
            self.device = device
            if device.type == "cuda":
                self._make_ctx()
        return self

    def cuda(self, device=None) -> "Network":
        return self.to(device="cuda" if device is None else device)

    def cpu(self) -> "Network":
        return self.to(device="cpu")

    def _make_ctx(self):
        if self._folded is None:
            raise RuntimeError("no weights loaded (get_model / load_state_dicts first)")
        self._ctx = _capi.Context(self.mc, self._folded, self.device.index, grn_exact=self.grn_exact)
        self._ctx.set_gemm_split(self._gemm_split)

    @property
    def gemm_split(self) -> bool:
        """The route of this network: its context's own state once it has one (whoever set it — `set_gemm_split`,
        `ctx.set_option("gemm_split", ...)`, `ctx.set_gemm_split`), else the route its context will be created on."""
        return self._ctx.get_gemm_split() if self._ctx is not None else self._gemm_split

    def set_gemm_split(self, enable: bool) -> "Network":
        """Route of THIS network's context: True = the large fp32 contractions as exact bf16x3 operand splits on the bf16 matrix
        cores (default), False = every product on the exact fp32 MFMA instruction.  Not to be called while another thread
        runs or captures a graph on this network."""
        self._gemm_split = bool(enable)
        if self._ctx is not None:
            self._ctx.set_gemm_split(self._gemm_split)
        return self

    def _drop_ctx(self):
        if self._ctx is not None:
            self._gemm_split = self._ctx.get_gemm_split()  # the route travels with the network to its next device
            self._ctx.close()
            self._ctx = None

    def min_grn_norm(self, reset: bool = False) -> float:
        """Validation mode only (grn_exact = True): the smallest per-clip GRN norm seen so far; the default fast path is exact
        for every input whose value here is >= 0.25."""
        if not self.grn_exact:
            raise RuntimeError("min_grn_norm() needs the validation mode: set network.grn_exact = True before .to(device)")
        return self.context().grn_min_norm(reset)

    def context(self) -> _capi.Context:
        if self._ctx is None:
            raise RuntimeError(
                "network is not on a GPU: call codec.network.to(device='cuda') first "
                "(l3ac_amd has no CPU path; the reference's PyTorch-CPU path is not part of this package)")
        return self._ctx

    # ---- reference Codec.preprocess (codec.py:79-84): kept for callers that use it -----------------
    def preprocess(self, audio_data: torch.Tensor):
        length = audio_data.shape[-1]
        hop = self.mc.hop_length
        pad_len = math.ceil(length / hop) * hop - length
        return torch.nn.functional.pad(audio_data, (0, pad_len)), length


class L3AC:
    """reference l3ac/__init__.py:84-121."""

    def __init__(self, config: L3ACConfig):
        self.config = config
        self.network = Network(config.network_config)

    def load_pretrained(self):
        """reference :104-106 minus the HTTP download (no network here): weights must already be on disk."""
        if not self.config.model_path.exists():
            raise FileNotFoundError(
                f"no weights at {self.config.model_path}: download "
                f"{self.config.weight_url.format('{encoder,quantizer,decoder,en_encoder,en_decoder}')} there, "
                "pass model_dir=..., or use get_model(..., synthetic_seed=N)")
        self.network.load_model(model_path=self.config.model_path)

    # ---- hot path -------------------------------------------------------------------------------------
    def _check_input(self, t: torch.Tensor, what: str):
        return check_codec_input(self.network, None, t, what)

    def _rate(self, sample_rate) -> Optional[int]:
        """None when `sample_rate` is absent or the codec's own rate (the plain path runs), else the validated rate."""
        if sample_rate is None or int(sample_rate) == self.config.sample_rate:
            return None
        resample_length(int(sample_rate), self.config.sample_rate, 1)  # unsupported rates raise before any device work
        return int(sample_rate)

    @torch.no_grad()
    def encode_audio(self, audio_data: torch.Tensor, validate: bool = False, sample_rate: Optional[int] = None, lengths=None):
        """audio (B, T) fp32 -> (q_feature (B, T_tok, C) fp32, {"indices": int32 (B, T_tok),
        "level_indices": fp32 (B, T_tok, D)}); the zero right-padding to a hop multiple happens in-kernel.
        ``sample_rate``: the rate of ``audio_data`` when it is not ``config.sample_rate``: the audio is first converted on the GPU,
        exactly as ``resample(audio_data, sample_rate, config.sample_rate)`` (T_tok then counts the converted samples).
        ``validate=True`` synchronises before and after the call: it raises — without running anything — if an EARLIER, unvalidated
        call on the context lost a cooperative transformer launch to its time limit, and raises if a launch of THIS call did.  Without
        it a later call on the context returns L3AC_ECOOP once, after the fact and possibly several calls late (the entry check does
        not synchronise: include/l3ac_hip.h, L3AC_ECOOP / l3ac_coop_timeout_pending).
        ``lengths``: B ints in 1..T, clips of different lengths in one call.  Samples at or after
        ``lengths[i]`` in row i are ignored, whatever they hold; clip i's first ``ceil(lengths[i] / hop)`` tokens are bit-identical
        to ``encode_audio(audio_data[i:i+1, :lengths[i]])``, the rest are zero, and the dict gains ``"lengths"``: those token counts
        (int32, on the CPU).  With ``sample_rate`` the lengths count samples at that rate."""
        if audio_data.dim() != 2:
            raise ValueError(f"audio_data must be (batch, samples), got {tuple(audio_data.shape)}")
        lens = None if lengths is None else ragged_lengths(lengths, audio_data.shape[0], audio_data.shape[1], "lengths")
        ctx = self._check_input(audio_data, "audio_data")
        rate = self._rate(sample_rate)
        if rate is not None and lens is not None:
            # each clip is converted as it would be alone: its zero padding, not its neighbour's samples, after its end
            audio_data = _zero_after(audio_data.to(torch.float32), lens)
            lens = [resample_length(rate, self.config.sample_rate, n) for n in lens]
        if rate is not None:
            audio_data = resample(audio_data, rate, self.config.sample_rate)
        audio = audio_data.to(torch.float32)
        if audio.stride(-1) != 1 or audio.stride(0) % 4 != 0 or audio.data_ptr() % 16 != 0:
            audio = audio.contiguous()
        b, t = audio.shape
        if t == 0 or b == 0:
            raise ValueError("empty audio")
        mc = self.network.mc
        dev = audio.device
        with torch.cuda.device(dev), validated(ctx, "encode_audio", validate):
            q_feature, indices, level_indices = encode_rows(ctx, audio, b, t, row_stride(audio), lens, torch.cuda.current_stream(dev).cuda_stream)
        if lens is not None:
            tok = torch.tensor([math.ceil(n / mc.hop_length) for n in lens], dtype=torch.int32)
            return q_feature, {"indices": indices, "level_indices": level_indices, "lengths": tok}
        return q_feature, {"indices": indices, "level_indices": level_indices}

    @torch.no_grad()
    def decode_audio(self, audio_feature: torch.Tensor = None, indices: torch.Tensor = None, validate: bool = False,
                     sample_rate: Optional[int] = None, lengths=None) -> torch.Tensor:
        """(B, T_tok, C) features, or int indices (B, T_tok) -> audio (B, T_tok * hop), not trimmed.
        ``sample_rate``: return the audio at this rate instead, exactly ``resample(decode_audio(...), config.sample_rate,
        sample_rate)``: (B, resample_length(config.sample_rate, sample_rate, T_tok * hop)), not trimmed either.
        Indices outside [0, codebook_size) — a corrupted or truncated token stream — are clamped into range and counted on
        the device (``codec.network.context().bad_index_count()``); with ``validate=True`` the call synchronises and raises
        if this call met any — or if a cooperative transformer launch of this call timed out (as encode_audio).
        ``lengths``: B token counts in 1..T_tok (``encode_audio(..., lengths=...)[1]["lengths"]``): clip i's first
        ``lengths[i] * hop`` samples are bit-identical to decoding its first ``lengths[i]`` tokens alone, the rest are zero; tokens
        after a clip's own are ignored (never counted as bad indices).  With ``sample_rate`` each clip is converted as it would be
        alone and is zero after ``resample_length(config.sample_rate, sample_rate, lengths[i] * hop)``."""
        src = audio_feature if audio_feature is not None else indices
        if src is None:
            raise ValueError("decode_audio needs audio_feature or indices")
        ctx = self._check_input(src, "decode input")
        rate = self._rate(sample_rate)
        mc = self.network.mc
        if audio_feature is not None:
            if audio_feature.dim() != 3 or audio_feature.shape[-1] != mc.feature_dim:
                raise ValueError(f"audio_feature must be (batch, tokens, {mc.feature_dim})")
            rows = audio_feature.to(torch.float32).contiguous()
        else:
            if indices.dim() != 2:
                raise ValueError("indices must be (batch, tokens)")
            rows = indices.to(torch.int32).contiguous()
        b, n_tok = rows.shape[:2]
        lens = None if lengths is None else ragged_lengths(lengths, b, n_tok, "lengths (tokens)")
        if min(lens or [n_tok]) * mc.en_coder_compress_rate < 2:
            # reference behaviour: the first EnhanceBlock's InstanceNorm1d (tconv/__init__.py:36) raises on a single frame
            raise ValueError(f"Expected more than 1 spatial element when training, got input size torch.Size([{b}, 4, 1])")
        bad_indices = None if audio_feature is not None else lambda bad: (
            f"{bad} of {b * n_tok} indices lie outside [0, {mc.codebook_size}): corrupted token stream")
        with torch.cuda.device(src.device), validated(ctx, "decode_audio", validate, bad_indices):
            audio = decode_rows(ctx, rows, audio_feature is not None, b, n_tok, lens, torch.cuda.current_stream(src.device).cuda_stream)
        if rate is None:
            return audio
        audio = resample(audio, self.config.sample_rate, rate)
        if lens is not None:  # each clip ends where its own converted samples end
            ends = [resample_length(self.config.sample_rate, rate, n * mc.hop_length) for n in lens]
            audio = _zero_after(audio, ends)
        return audio


    # ---- long audio (reference l3ac/codec.py:124-156, corrected: see l3ac_amd/chunking.py) ---------------------------
    def _batched(self, fn, chunks):
        """Run `fn` on chunks grouped by length: equal-length chunks (all the middle ones) go through ONE call as a batch."""
        out = [None] * len(chunks)
        by_len = {}
        for i, c in enumerate(chunks):
            by_len.setdefault(c.shape[-1] if c.dim() == 1 else c.shape[0], []).append(i)
        for idxs in by_len.values():
            res = fn(torch.stack([chunks[i] for i in idxs]))
            for k, i in enumerate(idxs):
                out[i] = res[k]
        return out

    @torch.no_grad()
    def extract_unit(self, audio_data: torch.Tensor, process_window: int = 5 * 16000, prefix_tokens: Optional[int] = None):
        """Encode a clip of any length window by window: (1, T) audio -> (ChunkData of indices, ChunkData of q_feature), the
        return structure and the default ``process_window`` of reference ``Codec.extract_unit`` (codec.py:124-147).  Unlike
        the reference, every chunk goes through the whole encode path (``en_encoder`` included); equal-length chunks are
        batched through one ``encode_audio`` call.  ``.data`` of either result is the merged token stream.

        ``prefix_tokens`` is the overlap of a chunk with its predecessor, in tokens.  **The default differs from the
        reference's**: the local attention's window (its look-back, ``en_coder_window_size`` tokens) instead of ONE hop, so
        the returned ``ChunkData.prefix_len`` is that window, not 1.  ``prefix_tokens=1`` gives exactly the reference's chunk
        geometry (``chunk_len = process_window // hop`` tokens, ``prefix_len = 1``): such ChunkData can be merged / decoded by
        reference code with the same arguments, and the reference's by ``decode_unit`` here."""
        assert audio_data.dim() == 2 and len(audio_data) == 1, "Only support batch size 1"  # codec.py:133
        mc = self.network.mc
        hop = mc.hop_length
        prefix_tokens = mc.en_coder_window_size if prefix_tokens is None else int(prefix_tokens)
        audio, _ = self.network.preprocess(audio_data)  # right zero-pad to a hop multiple (codec.py:79-84)
        chunk_len, prefix_len = _chunk_plan(hop, process_window, prefix_tokens)
        chunks = ChunkData(chunk_len=chunk_len, prefix_len=prefix_len, original_data=audio[0]).chunk_data
        idx, feat = [None] * len(chunks), [None] * len(chunks)

        def run(batch):
            q, ind = self.encode_audio(batch)
            return list(zip(ind["indices"], q))
        for i, (ix, q) in enumerate(self._batched(run, chunks)):
            idx[i], feat[i] = ix, q
        return (ChunkData(chunk_len=chunk_len // hop, prefix_len=prefix_tokens, chunk_data=idx),
                ChunkData(chunk_len=chunk_len // hop, prefix_len=prefix_tokens, chunk_data=feat))

    @torch.no_grad()
    def decode_unit(self, chunk_indices: Optional[ChunkData] = None, chunk_q_feature: Optional[ChunkData] = None,
                    audio_length: Optional[int] = None) -> torch.Tensor:
        """Decode what ``extract_unit`` returned, chunk by chunk (each with its overlap tokens as left context, equal-length
        chunks batched), and merge the waveforms: reference ``Codec.decode_unit`` (codec.py:149-156) -> (1, T) audio,
        trimmed to ``audio_length`` when given."""
        src = chunk_q_feature if chunk_q_feature is not None else chunk_indices
        if src is None:
            raise ValueError("decode_unit needs chunk_indices or chunk_q_feature")
        hop = self.network.mc.hop_length
        if chunk_q_feature is not None:
            waves = self._batched(lambda b: list(self.decode_audio(b)), src.chunk_data)
        else:
            waves = self._batched(lambda b: list(self.decode_audio(indices=b)), src.chunk_data)
        merged = ChunkData(chunk_len=src.chunk_len * hop, prefix_len=src.prefix_len * hop, chunk_data=waves).data[None, :]
        return merged if audio_length is None else merged[:, :audio_length]


    # ---- batches of long recordings through ragged chunk calls -------------------------------
    def _long_plan(self, process_window: int, prefix_tokens: Optional[int], chunks_per_call: Optional[int]):
        return window_args(self.network.mc, self.config.sample_rate, process_window, None if prefix_tokens is None else int(prefix_tokens),
                           chunks_per_call, _chunk_plan)

    @torch.no_grad()
    def encode_long(self, audio_data: torch.Tensor, lengths=None, process_window: int = 5 * 16000, prefix_tokens: Optional[int] = None,
                    sample_rate: Optional[int] = None, chunks_per_call: Optional[int] = None, validate: bool = False):
        """A batch of recordings of any lengths, window by window: audio (B, T) fp32 with ``lengths`` (B sample counts in 1..T; absent:
        every row is T long; samples at or after ``lengths[i]`` are ignored, whatever they hold) -> what
        ``encode_audio(..., lengths=)`` returns, in the same shapes: (q_feature (B, T_tok, C), {"indices": int32 (B, T_tok),
        "level_indices": fp32 (B, T_tok, D), "lengths": int32 CPU (B,)}), T_tok = ceil(T / hop), zero after a recording's own
        ``ceil(lengths[i] / hop)`` tokens.

        Row i equals ``extract_unit(audio_data[i:i+1, :lengths[i]], process_window, prefix_tokens)`` merged (``.data`` of the
        index and of the feature ChunkData) bit for bit; ``process_window`` and ``prefix_tokens`` mean what they mean there.  The
        chunks of the whole batch are cut on the device into the rows of ragged calls (``lengths=`` of encode_audio), at most
        ``chunks_per_call`` rows per call (default: 512 s of rows); the result does not depend on it.  ``sample_rate``: as
        encode_audio with ``lengths=`` (each recording converted as it would be alone, lengths counted at that rate).
        ``validate``: as encode_audio.  Capturable into a graph after ``context().reserve(chunks_per_call, row_samples)`` and one
        eager call: the plan and the lengths are host values fixed at capture."""
        return self._encode_long(audio_data, lengths, process_window, prefix_tokens, sample_rate, chunks_per_call, validate)[:2]

    def _encode_long(self, audio_data, lengths, process_window, prefix_tokens, sample_rate, chunks_per_call, validate):
        """``encode_long``, and third the recordings' sample counts at the codec's rate (``compress`` puts them into its headers)."""
        if audio_data.dim() != 2:
            raise ValueError(f"audio_data must be (batch, samples), got {tuple(audio_data.shape)}")
        if audio_data.shape[0] == 0 or audio_data.shape[1] == 0:
            raise ValueError("empty audio")
        lens = ragged_lengths([audio_data.shape[1]] * audio_data.shape[0] if lengths is None else lengths, audio_data.shape[0],
                              audio_data.shape[1], "lengths")
        chunk_len, prefix_tokens, per_call = self._long_plan(process_window, prefix_tokens, chunks_per_call)
        rate = self._rate(sample_rate)
        ctx = self._check_input(audio_data, "audio_data")
        refuse_grn_exact(self.network, "encode_long", "extract_unit")
        mc = self.network.mc
        hop = mc.hop_length
        audio = audio_data.to(torch.float32)
        if rate is not None:
            audio = resample(_zero_after(audio, lens), rate, self.config.sample_rate)
            lens = [resample_length(rate, self.config.sample_rate, n) for n in lens]
        audio = contiguous_rows(audio)
        b, t = audio.shape
        n_tok = math.ceil(t / hop)
        tok = [math.ceil(n / hop) for n in lens]
        cut = chunk_plan(lens, chunk_len, prefix_tokens * hop, hop)       # in samples, each recording padded to whole hops
        merge = chunk_plan(tok, chunk_len // hop, prefix_tokens, 1)       # the same chunks in tokens
        assert len(cut) == len(merge)
        dev = audio.device
        q_feature = torch.empty((b, n_tok, mc.feature_dim), dtype=torch.float32, device=dev)
        indices = torch.empty((b, n_tok), dtype=torch.int32, device=dev)
        level_indices = torch.empty((b, n_tok, len(mc.levels)), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev), validated(ctx, "encode_long", validate):
            stream = torch.cuda.current_stream(dev).cuda_stream
            for group in _chunk_groups(cut, per_call):
                samples = [cut[j].frames for j in group]
                longest = max(samples)
                rows = torch.empty((len(group), -(-longest // 4) * 4), dtype=torch.float32, device=dev)
                _chunk_cut(audio, _group_desc(cut, group), rows, stream)
                q, idx, li = encode_rows(ctx, rows, len(group), longest, rows.stride(0), samples, stream)
                desc = _group_desc(merge, group)
                _chunk_merge(q, desc, q_feature, stream)
                _chunk_merge(idx, desc, indices, stream)
                _chunk_merge(li, desc, level_indices, stream)
        return q_feature, {"indices": indices, "level_indices": level_indices, "lengths": torch.tensor(tok, dtype=torch.int32)}, lens

    @torch.no_grad()
    def decode_long(self, audio_feature: torch.Tensor = None, indices: torch.Tensor = None, lengths=None, process_window: int = 5 * 16000,
                    prefix_tokens: Optional[int] = None, sample_rate: Optional[int] = None, chunks_per_call: Optional[int] = None,
                    validate: bool = False) -> torch.Tensor:
        """The merged streams ``encode_long`` returns — (B, T_tok, C) features, or int indices (B, T_tok) — with ``lengths`` in tokens
        (absent: T_tok each) -> audio (B, T_tok * hop), not trimmed, zero after ``lengths[i] * hop``.

        Each recording's stream is cut the way ``ChunkData(cl, prefix_tokens, original_data=stream)`` cuts it
        (``cl = process_window // hop``), the chunks of the whole batch are decoded as rows of ragged calls (at most
        ``chunks_per_call`` per call; the result does not depend on it) and the waveforms merged, every chunk but a recording's
        first dropping its first ``prefix_tokens * hop`` samples: row i equals
        ``decode_unit(chunk_indices=ChunkData(cl, prefix_tokens, original_data=indices[i, :lengths[i]]))`` (or the
        ``chunk_q_feature`` form) bit for bit.  A chunk too short for the first EnhanceBlock raises the ValueError decode_audio
        raises, before any device work.  ``sample_rate``: as decode_audio with ``lengths=``.
        Out-of-range indices are clamped and counted as in decode_audio; tokens after a recording's own are never counted.  A token
        inside an overlap is decoded twice (as the last tokens of one chunk and as the prefix of the next) and is counted twice:
        ``validate=True`` raises when the count is non-zero and reports index OCCURRENCES in chunk rows, not distinct tokens."""
        src = audio_feature if audio_feature is not None else indices
        if src is None:
            raise ValueError("decode_long needs audio_feature or indices")
        mc = self.network.mc
        hop = mc.hop_length
        if audio_feature is not None:
            if audio_feature.dim() != 3 or audio_feature.shape[-1] != mc.feature_dim:
                raise ValueError(f"audio_feature must be (batch, tokens, {mc.feature_dim})")
        elif indices.dim() != 2:
            raise ValueError("indices must be (batch, tokens)")
        b, n_tok = src.shape[:2]
        if b == 0 or n_tok == 0:
            raise ValueError("empty token stream")
        tok = ragged_lengths([n_tok] * b if lengths is None else lengths, b, n_tok, "lengths (tokens)")
        chunk_len, prefix_tokens, per_call = self._long_plan(process_window, prefix_tokens, chunks_per_call)
        rate = self._rate(sample_rate)
        cut = chunk_plan(tok, chunk_len // hop, prefix_tokens, 1)
        if min(d.frames for d in cut) * mc.en_coder_compress_rate < 2:
            # reference behaviour, as decode_audio: the first EnhanceBlock's InstanceNorm1d raises on a single frame
            raise ValueError(f"Expected more than 1 spatial element when training, got input size torch.Size([{b}, 4, 1])")
        ctx = self._check_input(src, "decode input")
        refuse_grn_exact(self.network, "decode_long", "decode_unit")
        src = src.to(torch.float32 if audio_feature is not None else torch.int32).contiguous()
        dev = src.device
        audio = torch.empty((b, n_tok * hop), dtype=torch.float32, device=dev)
        bad_indices = None if audio_feature is not None else lambda bad: (
            f"{bad} index occurrences in the chunk rows (a token in an overlap counts twice) lie outside "
            f"[0, {mc.codebook_size}): corrupted token stream")
        with torch.cuda.device(dev), validated(ctx, "decode_long", validate, bad_indices):
            stream = torch.cuda.current_stream(dev).cuda_stream
            for group in _chunk_groups(cut, per_call):
                toks = [cut[j].frames for j in group]
                longest = max(toks)
                rows = torch.empty((len(group), longest) + tuple(src.shape[2:]), dtype=src.dtype, device=dev)
                _chunk_cut(src, _group_desc(cut, group), rows, stream)
                wave = decode_rows(ctx, rows, audio_feature is not None, len(group), longest, toks, stream)
                _chunk_merge(wave, _group_desc(cut, group, hop), audio, stream)
        if rate is None:
            return audio
        audio = resample(audio, self.config.sample_rate, rate)
        return _zero_after(audio, [resample_length(self.config.sample_rate, rate, n * hop) for n in tok])


    # ---- audio -> bytes -> audio (l3ac_amd/wire.py) --------------------------------------------
    @torch.no_grad()
    def compress(self, audio_data: torch.Tensor, lengths=None, sample_rate: Optional[int] = None, process_window: int = 5 * 16000,
                 prefix_tokens: Optional[int] = None, chunks_per_call: Optional[int] = None, validate: bool = False) -> list:
        """A batch of recordings -> one frame of bytes per recording: ``encode_long`` (its arguments, ``sample_rate`` and ``lengths``
        included), the ragged ``pack_indices``, one device-to-host copy.  A frame is ``wire.frame_header``'s 24 bytes followed by the
        recording's ``packed_bytes(n_tok, bits)`` bytes; its header carries the token count and the sample count at the codec's rate
        (after conversion, when ``sample_rate`` is given)."""
        _, info, samples = self._encode_long(audio_data, lengths, process_window, prefix_tokens, sample_rate, chunks_per_call, validate)
        mc = self.network.mc
        tok = info["lengths"].tolist()
        packed, nbytes = pack_indices(info["indices"], bits_per_token(mc), lengths=tok)
        host = packed.cpu().numpy()
        return [frame_header(mc, self.config.sample_rate, tok[i], samples[i]) + host[i, :k].tobytes() for i, k in enumerate(nbytes.tolist())]

    @torch.no_grad()
    def decompress(self, frames, sample_rate: Optional[int] = None, process_window: int = 5 * 16000, prefix_tokens: Optional[int] = None,
                   chunks_per_call: Optional[int] = None, validate: bool = False):
        """The frames of ``compress`` -> ``(audio (B, T) fp32, lengths int32 CPU)``: row i holds recording i's ``lengths[i]`` samples
        (its header's sample count; converted with ``resample_length`` when ``sample_rate`` is given) followed by zeros, T is their
        maximum.  Every frame is parsed and checked against this codec before any device work (``wire.parse_frame``: ValueError naming
        the field); then one upload, the ragged ``unpack_indices`` and ``decode_long`` (its arguments).  ``decompress(compress(x, n))``
        is ``decode_long(indices=encode_long(x, n)[1]["indices"], lengths=...)`` trimmed to the sample counts, bit for bit."""
        if isinstance(frames, (bytes, bytearray, memoryview)):
            raise ValueError("frames must be a sequence of frames, one per recording")
        mc = self.network.mc
        parsed = [parse_frame(f, mc, self.config.sample_rate) for f in frames]
        if not parsed:
            raise ValueError("no frames")
        rate = self._rate(sample_rate)
        bits = bits_per_token(mc)
        tok = [f.n_tok for f in parsed]
        n_tok = max(tok)
        host = torch.zeros((len(parsed), 4 * (-(-n_tok * bits // 32))), dtype=torch.uint8)
        for i, f in enumerate(parsed):
            host[i, :len(f.payload)] = torch.frombuffer(bytearray(f.payload), dtype=torch.uint8)
        self.network.context()  # raises when the network is not on a GPU
        indices = unpack_indices(host.to(self.network.device), n_tok, bits, lengths=tok)
        audio = self.decode_long(indices=indices, lengths=tok, process_window=process_window, prefix_tokens=prefix_tokens, sample_rate=sample_rate,
                                 chunks_per_call=chunks_per_call, validate=validate)
        samples = [f.n_samples if rate is None else resample_length(self.config.sample_rate, rate, f.n_samples) for f in parsed]
        return _zero_after(audio[:, :max(samples)], samples), torch.tensor(samples, dtype=torch.int32)

    # ---- quality of the round trip (l3ac_amd/metrics.py) ---------------------------------------
    @torch.no_grad()
    def evaluate(self, audio_data: torch.Tensor, lengths=None, sample_rate: Optional[int] = None, process_window: int = 5 * 16000,
                 prefix_tokens: Optional[int] = None, chunks_per_call: Optional[int] = None, scales=None, intelligibility: bool = False, loudness: bool = False,
                 pitch: bool = False, mcd: bool = False, lpc: bool = False, sdr: bool = False, bands: bool = False,
                 coherence: bool = False, r128: bool = False) -> dict:
        """How well this codec reproduces a batch of recordings: ``encode_long``, ``decode_long`` of the indices, then ``mel_distance``
        and ``signal_metrics`` between each recording and its decoded audio over the recording's own samples, all on the GPU.  With
        ``sample_rate`` the reference signal is the recording converted to the codec's rate (``resample``, each recording as it would
        be alone).  Returns ``mel_distance``'s and ``signal_metrics``' entries plus ``"tokens"`` (int32, CPU) and ``"bps"`` (fp64, CPU:
        ``bits_per_token * tokens / seconds``).  ``intelligibility=True`` adds ``"stoi"``, ``"estoi"`` and ``"stoi_frames"``: ``stoi``
        of the same pairs at the codec's rate.  ``loudness=True`` adds ``"loudness_reference"``,
        ``"loudness_decoded"`` and ``"loudness_shift"`` (decoded - reference, in LU): ``l3ac_amd.loudness`` of each side at the codec's
        rate (section 3.14).  ``pitch=True`` adds ``"f0_rmse_cents"``, ``"gpe"``, ``"vde"``, ``"ffe"``, ``"pitch_frames"`` and
        ``"pitch_voiced"`` (the frames voiced on both sides): ``l3ac_amd.pitch_metrics`` of the same pairs at the codec's rate with its
        default parameters (section 3.15).  ``mcd=True`` adds ``"mcd_db"``, ``l3ac_amd.mcd`` of the same pairs at the codec's rate with its
        default parameters (along the DTW path), and ``"mcd_plain_db"``, the same with ``dtw=False`` (frame f against frame f; both
        sides have the same lengths here) (section 3.17); a recording may then have at most 4096 frames of 160 samples.  ``lpc=True``
        adds ``"llr"``, ``"is_distance"``, ``"cepstral_distance_db"``, ``"seg_snr_db"`` and ``"lpc_frames"`` (the frames valid on both
        sides): ``l3ac_amd.lpc_metrics`` of the same pairs at the codec's rate with its default parameters (section 3.18); a recording
        may then have at most 16384 frames.  ``sdr=True`` adds ``"sdr_db"`` and ``"sdr_valid"``: ``l3ac_amd.sdr`` of the same pairs with
        its default parameters, the SDR of BSS Eval after a fitted distortion filter of 512 taps (section 3.21).  ``bands=True`` adds
        ``"fw_seg_snr_db"``, ``"wss"`` and ``"lsd_db"``: ``l3ac_amd.band_metrics`` of the same pairs at the codec's rate with its default
        parameters (section 3.22); a recording may then have at most 16384 frames.  ``coherence=True`` adds ``"csii"``, ``"csii_high"``,
        ``"csii_mid"``, ``"csii_low"`` and ``"csii_i3"``: ``l3ac_amd.csii`` of the same pairs at the codec's rate with its default parameters
        (section 3.23), under the same limit of 16384 frames.  ``r128=True`` adds ``"lra_reference"``, ``"lra_decoded"`` and ``"lra_shift"``
        (decoded - reference, in LU), ``l3ac_amd.loudness_range`` of each side, and ``"true_peak_reference_db"`` and
        ``"true_peak_decoded_db"`` in dBTP, ``l3ac_amd.true_peak`` of each side, at the codec's rate (section 3.25).  Every value equals
        composing those public calls by hand, bit for bit."""
        scales = _metric_scales(scales)
        if r128:  # a rate the meter or the oversampler is not defined for raises before any device work
            _check_loudness_rate(self.config.sample_rate)
            true_peak_factor(self.config.sample_rate)
        if coherence:  # a rate the defaults do not fit, or a batch too long for a pair, raises before any device work
            _, coh_frame, coh_hop, _, _ = _check_band_params(self.config.sample_rate, bands=sii_bands(self.config.sample_rate)[:2])
            longest = audio_data.shape[-1] if self._rate(sample_rate) is None else resample_length(int(sample_rate), self.config.sample_rate,
                                                                                                  max(audio_data.shape[-1], 1))
            if _lpc_frames(longest, coh_frame, coh_hop) > 16384:
                raise ValueError(f"evaluate(coherence=True): {longest} samples are more than the 16384 frames of a pair")
        if bands:  # a rate the defaults do not fit, or a batch too long for a pair, raises before any device work
            _, band_frame, band_hop, _, _ = _check_band_params(self.config.sample_rate, bands=None)
            longest = audio_data.shape[-1] if self._rate(sample_rate) is None else resample_length(int(sample_rate), self.config.sample_rate,
                                                                                                  max(audio_data.shape[-1], 1))
            if _lpc_frames(longest, band_frame, band_hop) > 16384:
                raise ValueError(f"evaluate(bands=True): {longest} samples are more than the 16384 frames of a pair")
        if lpc:  # a rate the defaults do not fit, or a batch too long for a pair, raises before any device work
            _, _, lpc_frame, lpc_hop = _check_lpc_params(self.config.sample_rate)
            longest = audio_data.shape[-1] if self._rate(sample_rate) is None else resample_length(int(sample_rate), self.config.sample_rate,
                                                                                                  max(audio_data.shape[-1], 1))
            if _lpc_frames(longest, lpc_frame, lpc_hop) > 16384:
                raise ValueError(f"evaluate(lpc=True): {longest} samples are more than the 16384 frames of a pair")
        if mcd:  # a rate the defaults do not fit, or a batch too long for a DTW pair, raises before any device work
            _check_mfcc_params(self.config.sample_rate, 512, _mfcc_hop(512, None), 40, 13)
            longest = audio_data.shape[-1] if self._rate(sample_rate) is None else resample_length(int(sample_rate), self.config.sample_rate,
                                                                                                  max(audio_data.shape[-1], 1))
            if 1 + longest // _mfcc_hop(512, None) > 4096:
                raise ValueError(f"evaluate(mcd=True): {longest} samples are more than the 4096 frames of a DTW pair")
        if pitch:  # a rate the tracker's defaults do not fit raises before any device work
            _check_pitch_params(self.config.sample_rate)
        if loudness:  # a rate the K-weighting is not defined for raises before any device work
            _check_loudness_rate(self.config.sample_rate)
        if intelligibility and self.config.sample_rate != 10000:  # a rate that cannot be taken to 10 kHz raises before any device work
            resample_length(self.config.sample_rate, 10000, 1)
        for n_fft, hop, n_mels in scales:  # unsupported scales raise before any device work
            _check_metric_params(self.config.sample_rate, n_fft, hop, n_mels)
        _, info, lens = self._encode_long(audio_data, lengths, process_window, prefix_tokens, sample_rate, chunks_per_call, False)
        rate = self._rate(sample_rate)
        reference = audio_data.to(torch.float32)
        if rate is not None:
            given = ragged_lengths([audio_data.shape[1]] * audio_data.shape[0] if lengths is None else lengths, audio_data.shape[0],
                                   audio_data.shape[1], "lengths")
            reference = resample(_zero_after(reference, given), rate, self.config.sample_rate)
        decoded = self.decode_long(indices=info["indices"], lengths=info["lengths"], process_window=process_window, prefix_tokens=prefix_tokens,
                                   chunks_per_call=chunks_per_call)[:, :reference.shape[1]]
        out = mel_distance(reference, decoded, sample_rate=self.config.sample_rate, scales=scales, lengths=lens)
        out.update(signal_metrics(reference, decoded, lengths=lens))
        if intelligibility:
            si = stoi(reference, decoded, sample_rate=self.config.sample_rate, lengths=lens)
            out.update({"stoi": si["stoi"], "estoi": si["estoi"], "stoi_frames": si["frames"]})
        if loudness:
            l_ref = _loudness(reference, sample_rate=self.config.sample_rate, lengths=lens)["lufs"]
            l_dec = _loudness(decoded, sample_rate=self.config.sample_rate, lengths=lens)["lufs"]
            out.update({"loudness_reference": l_ref, "loudness_decoded": l_dec, "loudness_shift": l_dec - l_ref})
        if r128:
            lra_ref = _loudness_range(reference, sample_rate=self.config.sample_rate, lengths=lens)["lra"]
            lra_dec = _loudness_range(decoded, sample_rate=self.config.sample_rate, lengths=lens)["lra"]
            out.update({"lra_reference": lra_ref, "lra_decoded": lra_dec, "lra_shift": lra_dec - lra_ref,
                        "true_peak_reference_db": _true_peak(reference, sample_rate=self.config.sample_rate, lengths=lens)["true_peak_db"],
                        "true_peak_decoded_db": _true_peak(decoded, sample_rate=self.config.sample_rate, lengths=lens)["true_peak_db"]})
        if pitch:
            pm = _pitch_metrics(reference, decoded, sample_rate=self.config.sample_rate, lengths=lens)
            out.update({"f0_rmse_cents": pm["f0_rmse_cents"], "gpe": pm["gpe"], "vde": pm["vde"], "ffe": pm["ffe"], "pitch_frames": pm["frames"],
                        "pitch_voiced": pm["voiced_both"]})
        if mcd:
            out["mcd_db"] = _mcd(reference, decoded, sample_rate=self.config.sample_rate, lengths=lens)["mcd_db"]
            out["mcd_plain_db"] = _mcd(reference, decoded, sample_rate=self.config.sample_rate, lengths=lens, dtw=False)["mcd_db"]
        if lpc:
            lm = _lpc_metrics(reference, decoded, sample_rate=self.config.sample_rate, lengths=lens)
            out.update({"llr": lm["llr"], "is_distance": lm["is_distance"], "cepstral_distance_db": lm["cepstral_distance_db"],
                        "seg_snr_db": lm["seg_snr_db"], "lpc_frames": lm["lpc_frames"]})
        if sdr:
            sd = _sdr(reference, decoded, lengths=lens)
            out.update({"sdr_db": sd["sdr_db"], "sdr_valid": sd["valid"]})
        if bands:
            bm = _band_metrics(reference, decoded, sample_rate=self.config.sample_rate, lengths=lens)
            out.update({"fw_seg_snr_db": bm["fw_seg_snr_db"], "wss": bm["wss"], "lsd_db": bm["lsd_db"]})
        if coherence:
            cs = _csii(reference, decoded, sample_rate=self.config.sample_rate, lengths=lens)
            out.update({"csii": cs["csii"], "csii_high": cs["csii_high"], "csii_mid": cs["csii_mid"], "csii_low": cs["csii_low"],
                        "csii_i3": cs["i3"]})
        tokens = info["lengths"]
        seconds = torch.tensor(lens, dtype=torch.float64) / self.config.sample_rate
        out["tokens"] = tokens
        out["bps"] = bits_per_token(self.network.mc) * tokens.to(torch.float64) / seconds
        return out

    # ---- streaming sessions (l3ac_amd/streaming.py) -------------------------------------------
    def stream_encoder(self, streams: int, process_window: int = 16000, prefix_tokens: Optional[int] = None,
                       chunks_per_call: Optional[int] = None) -> StreamEncoder:
        """A session of ``streams`` concurrent live streams: ``enc.push(audio, lengths=None, end=None)`` takes each stream's new
        samples and returns the tokens of the windows they complete — the bits ``encode_long`` gives the whole recording
        (``StreamEncoder.push``).  ``process_window``: the step in samples at the codec's rate, rounded down to whole hops as in
        ``extract_unit``, at least one hop.  ``prefix_tokens``: the look-back (default: the attention window, as everywhere else); it
        may be below, at or above the step, and 0 means independent windows.  ``chunks_per_call``: as in ``encode_long``.  The network
        must be on its GPU; a session belongs to the context it was created on.  There is no ``sample_rate=``: converting a live
        stream needs the filter's own carried state, which is a session of its own: put ``l3ac_amd.stream_resampler(streams, rate,
        config.sample_rate)`` in front (``StreamResampler``) for ``encode_long(..., sample_rate=rate)``'s bits."""
        return StreamEncoder(self, streams, process_window, prefix_tokens, chunks_per_call)

    def stream_decoder(self, streams: int, process_window: int = 16000, prefix_tokens: Optional[int] = None,
                       chunks_per_call: Optional[int] = None) -> StreamDecoder:
        """The decoding side: ``dec.push(audio_feature=None, indices=None, lengths=None, end=None)`` takes each stream's new tokens
        and returns the audio of the windows they complete — ``decode_long``'s bits (``StreamDecoder.push``).  The step is
        ``process_window // hop`` tokens; the other arguments as in ``stream_encoder``."""
        return StreamDecoder(self, streams, process_window, prefix_tokens, chunks_per_call)


def set_gemm_split(enable: bool) -> None:
    """Route the large fp32 channel contractions of EVERY live network (and of networks created later) through the bf16x3
    split-operand kernels (default, fp32 accuracy on the bf16 matrix cores) or through the exact v_mfma_f32_32x32x2_f32
    kernel.  The state itself lives in each network's context (``Network.set_gemm_split``, l3ac_ctx_set_gemm_split): graphs
    already captured keep the route they were captured on."""
    global _default_gemm_split
    _default_gemm_split = bool(enable)
    for net in list(_networks):
        net.set_gemm_split(enable)


def get_gemm_split() -> bool:
    """The DEFAULT route: what networks created from now on start with (``L3AC_GEMM_SPLIT`` read the way the library reads it, or
    the last module-level ``set_gemm_split``).  It is not the state of any live network — a network whose route was changed on
    its own (``Network.set_gemm_split``, a context option) reports it in ``network.gemm_split``.  Code that switches routes
    temporarily should save and restore per network, or use ``gemm_split_routes()``."""
    return _default_gemm_split


def gemm_split_routes() -> dict:
    """{network: route} of every live network — the snapshot ``restore_gemm_split_routes`` takes back."""
    return {net: net.gemm_split for net in list(_networks)}


def restore_gemm_split_routes(routes: dict, default: Optional[bool] = None) -> None:
    """Undo a module-level ``set_gemm_split``: every network in `routes` gets ITS previous route back (a module-level
    ``set_gemm_split(before)`` would overwrite individually routed networks with the default)."""
    global _default_gemm_split
    if default is not None:
        _default_gemm_split = bool(default)
    for net, route in routes.items():
        net.set_gemm_split(route)


def stream_packer(streams: int, bits: int) -> StreamPacker:
    """A session that packs the tokens of ``streams`` concurrent live streams into the bytes of the wire, push by push:
    ``packed, n_bytes = packer.push(indices, lengths=None, end=None)``.  However a stream's tokens are split over pushes, what it emits
    adds up to the first ``packed_bytes(n, bits)`` bytes of ``pack_indices`` of the whole stream (``StreamPacker.push``).  ``bits`` in
    8..32 (``bits_per_token``: 17 and 18 for the shipped models).  Needs no codec; the state lives on the device of the first push."""
    return StreamPacker(streams, bits)


def stream_unpacker(streams: int, bits: int) -> StreamUnpacker:
    """The receiving side: ``indices, n_tok = unpacker.push(packed, lengths=None, end=None)`` takes any run of each stream's bytes and
    returns the tokens they complete; what a stream emits adds up to ``unpack_indices`` of the whole stream (``StreamUnpacker.push``)."""
    return StreamUnpacker(streams, bits)


def ragged_lengths(lengths, batch: int, limit: int, what: str = "lengths") -> list:
    """``lengths=`` of encode_audio / decode_audio as B Python ints in 1..limit; raises ValueError (before any device work)
    otherwise.  Accepts a sequence, a NumPy array or a tensor (a CUDA tensor is copied to the host)."""
    return int_list(lengths, batch, 1, limit, what, f"a batch of {batch}")


def stream_resampler(streams: int, orig_sr: int, target_sr: int) -> StreamResampler:
    """A session that converts ``streams`` concurrent live streams from ``orig_sr`` to ``target_sr`` packet by packet:
    ``y, n = rs.push(audio, lengths=None, end=None)`` takes each stream's new samples and returns the converted samples they complete.
    However a stream is split over pushes, what it emits adds up to ``resample`` of the whole stream, bit for bit, and to
    ``resample_length`` samples once it has ended (``StreamResampler.push``).  Needs no codec; it composes with the codec's sessions::

        rs  = l3ac.stream_resampler(S, 48000, codec.config.sample_rate)
        enc = codec.stream_encoder(streams=S, process_window=16000)
        y, n = rs.push(packet_48k, lengths=new_samples, end=finished)
        q_feature, indices = enc.push(y, lengths=n, end=finished)        # encode_long(..., sample_rate=48000)'s bits
        # decoding side
        wave, n_tok = dec.push(indices=..., lengths=..., end=finished)
        out, n_out = rs_out.push(wave, lengths=n_tok * hop, end=finished)  # decode_long(..., sample_rate=44100)'s bits

    Rates are checked here (``resample_length``'s errors); the state lives on the device of the first push."""
    return StreamResampler(streams, orig_sr, target_sr)


def stream_filter(streams: int, sos, dtype: torch.dtype = torch.float32) -> StreamFilter:
    """A session that runs ``streams`` concurrent live streams through the cascade ``sos`` (``sosfilt``'s (N, 6) rows) packet by packet:
    ``y, n = flt.push(audio, lengths=None, end=None)`` returns each stream's new samples filtered, as many as it was given.  However
    a stream is split over pushes, what it emits adds up to ``sosfilt`` of the whole stream, bit for bit (``StreamFilter.push``).  Needs
    no codec; ``sos`` is checked here (``sosfilt``'s errors); the state lives on the device of the first push."""
    return StreamFilter(streams, sos, dtype)


def get_model(config_name, model_dir=None, synthetic_seed: Optional[int] = None, synthetic_profile: str = "mild") -> L3AC:
    """reference l3ac/__init__.py:21-25.  ``config_name`` is a shipped model name (``list_models()``) or a path
    to a TOML file of the same schema.  Weights come from ``{model_dir}/{name}.{version}/*.pt`` (default
    ``~/.cache/l3ac``, the reference's cache), or — with ``synthetic_seed`` — from the seeded generator
    (``synthetic_profile``: "mild", or "stress" = the statistics of a trained network, see ``weights.synthetic_state_dicts``)."""
    overrides = {} if model_dir is None else {"model_dir": Path(model_dir)}
    codec = L3AC(L3ACConfig(config_file=resolve_config_file(config_name), **overrides))
    if synthetic_seed is not None:
        codec.network.load_state_dicts(_weights.synthetic_state_dicts(codec.config.network_config, seed=synthetic_seed,
                                                                      profile=synthetic_profile))
    else:
        codec.load_pretrained()
    return codec


def get_model_info(model, eval_flops_seconds=10, sample_rate: int = 16000) -> dict:
    """reference l3ac/__init__.py:28-51.  ``model`` is ``codec.network`` (as in example.py:11) or the codec.  The reference
    traces the model with ptflops on ``eval_flops_seconds`` of audio; here ``macs`` is the analytic multiply-accumulate
    count of the same input (l3ac_amd/macs.py: every conv / linear product plus the local-attention products, which
    ptflops does not see), ``macs_breakdown`` its parts, and ``params`` the exact parameter count of the five modules."""
    from .macs import path_macs
    mc = model.mc if hasattr(model, "mc") else model.network.mc
    compress_rate = mc.hop_length
    codebook_size = mc.codebook_size
    frame_rate = sample_rate / compress_rate
    params = sum(int(math.prod(shape)) for m in _weights.MODULE_NAMES for _, shape in _weights.raw_keys(mc, m))
    macs = path_macs(mc, int(eval_flops_seconds * sample_rate))
    return {
        "macs": macs["total"],
        "macs_breakdown": macs,
        "params": params,
        "codebook_size": codebook_size,
        "frame_rate": frame_rate,
        "bps": frame_rate * math.log2(codebook_size),
        "receptive_field": mc.en_coder_window_size / frame_rate,
    }
