"""Feature front-end on the HIP device: waveform -> normalised log-mel features in the model's input layout.

Mirrors the transform chain of the reference's TIMIT loader (reference training/torch/timit.py:78-97):

    torchaudio.transforms.MelSpectrogram(sample_rate=16000, win_length=400, hop_length=160, n_mels=80)
    torch.log
    (x - mean) / (variance + eps)        # NB: the variance, not its square root (timit.py:83), eps = 1e-3

with torchaudio's defaults spelled out: n_fft = 400, centred frames with reflect padding, periodic Hann window, power 2,
HTK mel scale between 0 and sample_rate / 2, no filterbank normalisation.  The reference applies the chain per utterance and
zero-pads the FEATURES of a batch (timit.py:54-69, 96-103); ``lengths`` reproduces that for a zero-padded batch of waveforms.

All arithmetic runs in libnbasr_hip.so (frontend.hip + the fp32 MFMA GEMM); there is no CPU path.
"""
import math

import numpy as np
import torch

from . import hip


def hz_to_mel_htk(f):
    return 2595.0 * np.log10(1.0 + np.asarray(f, dtype=np.float64) / 700.0)


def mel_to_hz_htk(m):
    return 700.0 * (10.0 ** (np.asarray(m, dtype=np.float64) / 2595.0) - 1.0)


def mel_filterbank(n_freqs, n_mels, sample_rate, f_min=0.0, f_max=None):
    """(n_freqs, n_mels) triangular HTK filterbank, torchaudio.functional.melscale_fbanks(norm=None, mel_scale='htk')."""
    f_max = sample_rate / 2.0 if f_max is None else f_max
    all_freqs = np.linspace(0.0, sample_rate // 2, n_freqs)
    f_pts = mel_to_hz_htk(np.linspace(hz_to_mel_htk(f_min), hz_to_mel_htk(f_max), n_mels + 2))
    f_diff = f_pts[1:] - f_pts[:-1]
    slopes = f_pts[None, :] - all_freqs[:, None]
    down = -slopes[:, :-2] / f_diff[:-1]
    up = slopes[:, 2:] / f_diff[1:]
    return np.maximum(0.0, np.minimum(down, up))


def windowed_dft_matrix(n_fft, win_length):
    """(2 * (n_fft/2 + 1), n_fft): rows 0..n_fft/2 = w[n] cos(2 pi k n / N), then the same with -sin (periodic Hann w)."""
    n = np.arange(n_fft, dtype=np.float64)
    window = np.zeros(n_fft)
    left = (n_fft - win_length) // 2
    window[left:left + win_length] = 0.5 - 0.5 * np.cos(2.0 * math.pi * np.arange(win_length) / win_length)
    k = np.arange(n_fft // 2 + 1, dtype=np.float64)[:, None]
    ang = 2.0 * math.pi * k * n[None, :] / n_fft
    return np.concatenate([np.cos(ang) * window, -np.sin(ang) * window], axis=0)


# ---- which frames of a waveform stream are final (pure python; hop <= win / 2) -------------------------------------------------------
# Frame t covers samples [hop t - win/2, hop t + win/2), negative indices reflected (i -> -i) and, once the length L is known,
# i >= L -> 2 (L - 1) - i; an utterance of L > win/2 samples has L // hop + 1 frames.
def frames_final(samples, hop=160, win=400):
    """Frames that can no longer change after ``samples`` samples, while the end is unknown: those with hop t + win/2 <= samples.
    Frame 0 reflects sample win/2 into its left half, so it needs one sample more."""
    half = win // 2
    return 0 if samples <= half else (samples - half) // hop + 1


def frames_total(samples, hop=160, win=400):
    """Frames of an utterance of ``samples`` samples (its last frame is never final earlier: a flush emits 1 or 2 frames)."""
    if samples <= win // 2:
        raise ValueError(f'reflect padding needs more than {win // 2} samples (the utterance has {samples})')
    return samples // hop + 1


def frames_peek(samples, hop=160, win=400):
    """Frames a peek of the stream returns after ``samples`` samples: those a flush would emit now (1 or 2), and none while the utterance
    is too short to be ended (``frames_total`` refuses it: a peek ends nothing, so it has nothing to refuse)."""
    return 0 if samples <= win // 2 else frames_total(samples, hop, win) - frames_final(samples, hop, win)


def retain_from(frames_emitted, hop=160, win=400):
    """First sample a stream must keep once ``frames_emitted`` frames are out.  One more than the next frame's left edge: when the
    length turns out to be a multiple of hop, the last frame's end reflection reaches back to sample L - win/2 - 1.  With
    ``frames_emitted = frames_final(L)`` this keeps at most ``win`` samples."""
    return max(0, hop * frames_emitted - win // 2 - 1)


# ---- the resampler's geometry (pure python, integers only; DESIGN.md 9 "Resampler") ---------------------------------------------------
# o = orig / gcd, n = new / gcd.  Output j sums the samples m with |m n - j o| <= reach: the integer form of |t| < 6 for
# t = (m / o - j / n) 0.99 min(o, n).  Everything below follows from that one rule, so host, model and kernel agree on the support.
RESAMPLE_MAX_RATIO = 1024          # the kernel's limits (include/nbasr.h): reduced rates, and taps of the largest support
RESAMPLE_MAX_TAPS = 48


def resample_ratio(orig_freq, new_freq):
    """(o, n): the two rates with their common factor taken out."""
    orig_freq, new_freq = int(orig_freq), int(new_freq)
    if orig_freq <= 0 or new_freq <= 0:
        raise ValueError(f'sample rates must be positive (got {orig_freq} -> {new_freq})')
    g = math.gcd(orig_freq, new_freq)
    return orig_freq // g, new_freq // g


def resample_reach(o, n):
    """The largest |m n - j o| inside the support: the largest integer d with d min(o, n) 99 < 600 o n."""
    return (600 * o * n - 1) // (99 * min(o, n))


def resample_support(j, o, n):
    """(first, last) sample of output j's support (before clipping to the utterance)."""
    d = resample_reach(o, n)
    return -((d - j * o) // n), (j * o + d) // n


def resample_taps(o, n):
    """Taps of the largest support over the n phases (the support of output j + n is that of j moved by o samples)."""
    return max(hi - lo + 1 for lo, hi in (resample_support(p, o, n) for p in range(n)))


def resample_total(samples, o, n):
    """Outputs of an utterance of ``samples`` samples: ceil(n samples / o)."""
    return -(-n * samples // o)


def resample_final(samples, o, n):
    """Outputs that can no longer change after ``samples`` samples, while the end is unknown: those whose last supported sample has
    arrived, (j o + reach) // n < samples.  Per output, not per block of o samples."""
    return max(0, (samples * n - resample_reach(o, n) - 1) // o + 1)


def resample_peek(samples, o, n):
    """Outputs a peek returns after ``samples`` samples: those a flush would emit now."""
    return resample_total(samples, o, n) - resample_final(samples, o, n)


def resample_retain_from(outputs_emitted, o, n):
    """First sample a stream must keep once ``outputs_emitted`` outputs are out: the first of the next output's support."""
    return max(0, resample_support(outputs_emitted, o, n)[0])


def _resample_states(o, n):
    """Sample counts that show every state of a stream: samples -> samples + o moves every count by n outputs and every support by o
    samples, so one period is all there is once the next output's support no longer starts before sample 0 (the support is
    2 reach / n samples wide)."""
    return range(0, 2 * resample_reach(o, n) // n + 2 * o + 2)


def resample_tail_capacity(o, n):
    """The most samples a stream retains: the largest ``samples - resample_retain_from(resample_final(samples))``."""
    return max(s - resample_retain_from(resample_final(s, o, n), o, n) for s in _resample_states(o, n))


def resample_max_pending(o, n):
    """The most outputs a flush or a peek returns (the outputs still pending at an arbitrary cut)."""
    return max(resample_peek(s, o, n) for s in _resample_states(o, n))


def resample_lookahead(o, n):
    """Samples an output waits for beyond its own instant j o / n: ceil(reach / n)."""
    return -(-resample_reach(o, n) // n)


def resample_table(o, n):
    """(n, taps | 1) float64 coefficients: row p, element i belongs to sample lo(p) + i of output p (and to lo(p) + i + k o of output
    p + k n); zero beyond the row's support.  The odd pitch is the kernel's (LDS banks)."""
    taps, base = resample_taps(o, n), 0.99 * min(o, n)
    table = np.zeros((n, taps | 1))
    for p in range(n):
        lo, hi = resample_support(p, o, n)
        t = (np.arange(lo, hi + 1) * n - p * o).astype(np.float64) * (base / (o * n))      # (m / o - p / n) base, the difference exact
        table[p, :hi - lo + 1] = (base / o) * np.sinc(t) * np.cos(math.pi * t / 12.0) ** 2
    return table


def end_frames_bound(pending=0, hop=160, win=400):
    """The most frames the front-end emits for the end of an utterance when up to ``pending`` more samples arrive with it (a
    resampler's flush): the largest ``frames_total(s + pending) - frames_final(s)``.  2 without a resampler."""
    return (hop - 1 + win // 2 + pending) // hop


class LogMelFrontend:
    """``frontend(wave, lengths=None) -> (B, n_mels, T)`` float32 on ``wave``'s HIP device, ``T = L // hop + 1``.

    ``wave``: (B, L) float32 device tensor (zero-padded batch); ``lengths``: per-utterance sample counts (sequence or int32
    tensor) or None.  ``mean`` / ``variance``: per-mel statistics (the reference's ``timit_train_stats.npz`` arrays
    ``moving_mean`` / ``moving_variance``); None = no normalisation (plain log-mel)."""

    def __init__(self, sample_rate=16000, win_length=400, hop_length=160, n_mels=80, n_fft=None, mean=None, variance=None,
                 eps=1e-3, device='cuda:0'):
        self.sample_rate, self.win_length, self.hop_length, self.n_mels = sample_rate, win_length, hop_length, n_mels
        self.n_fft = win_length if n_fft is None else n_fft
        if self.n_fft % 4:
            raise ValueError('n_fft must be a multiple of 4 (GEMM K alignment)')
        self.device = torch.device(device)
        self.bins = self.n_fft // 2 + 1
        self.bins_padded = (self.bins + 3) // 4 * 4
        dft = windowed_dft_matrix(self.n_fft, win_length)
        fb = np.zeros((n_mels, self.bins_padded))
        fb[:, :self.bins] = mel_filterbank(self.bins, n_mels, sample_rate).T
        mean = np.zeros(n_mels) if mean is None else np.asarray(mean, dtype=np.float64)
        inv = np.ones(n_mels) if variance is None else 1.0 / (np.asarray(variance, dtype=np.float64) + eps)
        if mean.shape != (n_mels,) or inv.shape != (n_mels,):
            raise ValueError(f'mean and variance must have {n_mels} entries')
        f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(self.device)
        self.dft, self.fbank, self.mean, self.inv_scale = f32(dft), f32(fb), f32(mean), f32(inv)
        self.zero_bias = torch.zeros(max(2 * self.bins, n_mels), device=self.device)

    def num_frames(self, samples):
        return samples // self.hop_length + 1 if samples > 0 else 0

    def stream(self, batch):
        """A ``FrontendStream``: this front-end push by push for a lockstep batch of ``batch`` waveform streams."""
        return FrontendStream(self, batch)

    def stream_images(self):
        """(dft image, fbank image) of nbasr_frontend_stream_step: the two matrices, rows padded to 208 bins, in the order the lanes of
        the fp32 MFMA read them (include/nbasr.h).  Built once, shared by every stream of this front-end."""
        if getattr(self, '_images', None) is None:
            if (self.win_length, self.n_fft, self.hop_length, self.n_mels) != (400, 400, 160, 80):
                raise ValueError('the streaming front-end is built for win = n_fft = 400, hop = 160, 80 mel bands')
            rows = 208
            dft = self.dft.cpu().numpy()                                         # the float32 values __call__ multiplies by
            m = np.zeros((2, rows, self.n_fft), dtype=np.float32)
            m[0, :self.bins], m[1, :self.bins] = dft[:self.bins], dft[self.bins:]
            # (part, tile, row i, block, s, q) -> [tile][part][block][lane = 16 q + i][s]: element s of lane l holds k = 16 kb + 4 s + (l >> 4)
            dft_image = m.reshape(2, rows // 16, 16, self.n_fft // 16, 4, 4).transpose(1, 0, 3, 5, 2, 4)
            fb = np.zeros((self.n_mels, rows), dtype=np.float32)
            fb[:, :self.bins] = self.fbank.cpu().numpy()[:, :self.bins]
            fb_image = fb.reshape(self.n_mels // 16, 16, rows // 16, 4, 4).transpose(0, 2, 4, 1, 3)
            dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).reshape(-1).to(self.device)
            self._images = (dev(dft_image), dev(fb_image))
        return self._images

    def __call__(self, wave, lengths=None):
        if wave.dim() != 2 or wave.dtype != torch.float32 or not wave.is_cuda:
            raise hip.HipError('wave must be a (batch, samples) float32 tensor on a HIP device; this package has no CPU path')
        wave = wave.contiguous()
        b, samples = wave.shape
        if lengths is not None and not torch.is_tensor(lengths):
            lengths = torch.tensor(list(lengths), dtype=torch.int32)
        if lengths is not None:
            if int(lengths.max()) > samples or int(lengths.min()) <= self.n_fft // 2:
                raise ValueError(f'lengths must lie in ({self.n_fft // 2}, {samples}]')
            lengths = lengths.to(device=wave.device, dtype=torch.int32).contiguous()
        t = self.num_frames(samples)
        ld = hip.round_up4(t)
        frames = torch.empty(b, self.n_fft, ld, device=wave.device)
        hip.frame_signal(wave, lengths, frames, self.n_fft, self.hop_length)
        spec = torch.empty(b, 2 * self.bins, ld, device=wave.device)
        hip.pointwise_linear(frames, t, self.dft, self.zero_bias, spec)
        power = torch.empty(b, self.bins_padded, ld, device=wave.device)
        hip.power_spectrum(spec, self.bins, power)
        mel = torch.empty(b, self.n_mels, ld, device=wave.device)
        hip.pointwise_linear(power, t, self.fbank, self.zero_bias, mel)
        hip.log_normalize(mel, lengths, self.mean, self.inv_scale, mel, samples, self.hop_length)
        return mel[:, :, :t] if ld != t else mel


class _SampleTailStream:
    """A lockstep batch of waveform streams whose state is two sample tails, used in turn: what ``FrontendStream`` and
    ``ResamplerStream`` share (csrc/sample_tail.h is the C side's half).  ``_tails[_turn]`` (batch, ``pitch`` rounded up to 4) holds
    samples ``_tail_first`` .. ``_tail_first + _tail_len - 1`` of every utterance; ``samples_in`` counts what was pushed.  A step reads
    that tail and the new samples; the step that ends a push copies what the next one needs into the OTHER tail, which becomes the
    current one; the step that ends the utterance, a peek's included, retains nothing.  A subclass adds its output counter, the
    launch, and which sample is the first that the next step still needs."""

    def __init__(self, batch, device, pitch):
        batch = int(batch)
        if batch < 1:
            raise ValueError(f'batch must be positive (got {batch})')
        self.batch, self.device = batch, device
        self._tails = torch.zeros(2, batch, hip.round_up4(pitch), device=device)
        self._tail = tuple(self._tails)           # the two tails as views made once: a step indexes a tuple, not a tensor
        self.state_bytes = self._tails.numel() * self._tails.element_size()

    def reset(self):
        """Start the next batch of utterances; the tails are re-used."""
        self.samples_in = self._tail_first = self._tail_len = self._turn = 0
        self._flushed = False

    def _admit(self, wave):
        if self._flushed:
            raise ValueError('push after flush: call reset() to start the next utterance')
        if not isinstance(wave, torch.Tensor) or wave.dim() != 2 or wave.shape[0] != self.batch:
            raise ValueError(f'expected a ({self.batch}, samples) chunk, got {tuple(getattr(wave, "shape", ()))}')
        if wave.dtype != torch.float32 or wave.device != self.device:
            raise ValueError(f'the chunk must be float32 on {self.device} (got {wave.dtype} on {wave.device})')
        wave, n = wave.detach(), wave.shape[1]
        if n and (wave.stride(1) != 1 or (self.batch > 1 and wave.stride(0) < n)):
            wave = wave.contiguous()
        return wave

    def _turns(self, n, commit, final):
        """Where does a step of ``n`` new samples read, and where, if anywhere, does it retain?  -> (tail_in, tail_out or None).  An empty
        push leaves the tail where it is: nothing to copy.  The subclass works out the first retained sample only for a step that
        retains (``ResamplerStream``'s form of the rule; ``FrontendStream`` did so for an empty committed push as well, and never read
        it: such a push completes no frame -- the push before it emitted every final one -- and launches nothing)."""
        turn = self._turn
        return self._tail[turn], (self._tail[turn ^ 1] if commit and not final and n else None)

    def _retained(self, n, tail_out, new_first):
        """Commit a step: its ``n`` samples are in, and the tail it wrote, if any, is the current one."""
        self.samples_in += n
        if tail_out is not None:
            self._turn ^= 1
            self._tail_first = new_first
            self._tail_len = self.samples_in - new_first


class FrontendStream(_SampleTailStream):
    """``LogMelFrontend`` push by push (``LogMelFrontend.stream``): one fused HIP launch per push, state carried in two sample tails.

        fs = frontend.stream(batch=B)
        for chunk in waveform_chunks:              # (B, n) float32 on the device, any n >= 0
            feats = fs.push(chunk)                 # (B, 80, m): the frames that are final now (frames_final)
        last = fs.flush()                          # (B, 80, 1 or 2): the frames that needed the utterance's end
        # fs.peek() at any point before: the frames flush() would return then, the stream left as it was
        # torch.cat([*pushes, last], 2) has the L // 160 + 1 frames of frontend(whole waveform); the bits do not depend on the chunking

    ``out=(tensor, col0)``: write the frames into columns ``col0`` .. of a caller's contiguous (B, 80, ld) float32 tensor (ld % 4 == 0)
    and return that view.  The batch is lockstep: every lane receives the same number of samples.  Apart from returned features all
    memory is allocated here (``state_bytes``: the two tails of 404 samples per lane; the matrices belong to the front-end).  The
    tails and their turn-taking are ``_SampleTailStream``'s."""

    def __init__(self, frontend, batch):
        self.frontend = frontend
        self.hop, self.win = frontend.hop_length, frontend.n_fft
        super().__init__(batch, frontend.device, self.win + 1)
        self.lookahead_samples = self.win // 2
        self._dft_image, self._fbank_image = frontend.stream_images()
        assert self.state_bytes == hip.frontend_stream_state_bytes(self.batch, self.win)
        self.reset()

    def reset(self):
        """Start the next batch of utterances; the tails are re-used."""
        super().reset()
        self.frames_out = 0

    # ---- public ----------------------------------------------------------------------------------------------------------------
    def push(self, wave_chunk, out=None):
        """Feed (batch, n) samples; returns the (batch, 80, m) frames that became final, m = frames_final(samples_in) - frames_out."""
        wave = self._admit(wave_chunk)
        m = frames_final(self.samples_in + wave.shape[1], self.hop, self.win) - self.frames_out
        feats, col0, view = self._destination(out, m)
        self._step(wave, m, feats, col0, self.frames_out, True, False)
        return view

    def push_tiled(self, wave_chunk, out, max_frames):
        """``push`` for a caller that consumes at most ``max_frames`` frames at a time from one buffer: a generator that writes the next
        frames to columns 0 .. of ``out`` and yields their count (once, with 0, when the push completes no frame).  Drain it: the stream
        advances with the last launch."""
        wave = self._admit(wave_chunk)
        m = frames_final(self.samples_in + wave.shape[1], self.hop, self.win) - self.frames_out
        first = self.frames_out
        for off in range(0, max(m, 1), max_frames):
            k = min(max_frames, m - off)
            feats, col0, _ = self._destination((out, 0), k)
            self._step(wave, k, feats, col0, first + off, off + k == m, False)
            yield k

    def flush(self, out=None):
        """End the utterance: its last 1 or 2 frames, with the end's reflect padding."""
        if self._flushed:
            raise ValueError('flush called twice: call reset() to start the next utterance')
        m = frames_total(self.samples_in, self.hop, self.win) - self.frames_out
        feats, col0, view = self._destination(out, m)
        self._step(None, m, feats, col0, self.frames_out, True, True)
        self._flushed = True
        return view

    def peek(self, out=None, extra=None):
        """The frames ``flush()`` would return now (``frames_peek``: 1 or 2, none in the utterance's first ``win // 2`` samples), with the
        stream left as it was: the launch that ends an utterance retains nothing, and nothing advances.  ``extra``: (batch, n)
        uncommitted samples, taken as if pushed and then ended -- the frames ``push(extra)`` and ``flush()`` would return together."""
        if self._flushed:
            raise ValueError('peek after flush: call reset() to start the next utterance')
        if extra is None or extra.shape[-1] == 0:
            extra = None
            m = frames_peek(self.samples_in, self.hop, self.win)      # (== frames_total - frames_out: a push emits every final frame)
        else:
            extra = self._admit(extra)
            total = self.samples_in + extra.shape[1]
            m = 0 if total <= self.win // 2 else frames_total(total, self.hop, self.win) - self.frames_out
        feats, col0, view = self._destination(out, m)
        if m:
            self._step(extra, m, feats, col0, self.frames_out, False, True)
        return view

    # ---- one launch ------------------------------------------------------------------------------------------------------------
    def _destination(self, out, m):
        """(tensor the launch writes, first column, the view of the m frames)."""
        fe = self.frontend
        if out is None:
            buf = torch.empty(self.batch, fe.n_mels, hip.round_up4(m), device=self.device)
            return buf, 0, (buf[:, :, :m] if buf.shape[2] != m else buf)
        buf, col0 = out
        col0 = int(col0)
        if (not isinstance(buf, torch.Tensor) or buf.dim() != 3 or buf.shape[0] != self.batch or buf.shape[1] != fe.n_mels or buf.shape[2] % 4
                or buf.dtype != torch.float32 or buf.device != self.device or not buf.is_contiguous()):
            raise ValueError(f'out must be a contiguous float32 ({self.batch}, {fe.n_mels}, ld) tensor on {self.device}, ld a multiple of 4')
        if col0 < 0 or col0 + m > buf.shape[2]:
            raise ValueError(f'out holds {buf.shape[2]} columns: {m} frames do not fit at column {col0}')
        return buf, col0, buf[:, :, col0:col0 + m]

    def _step(self, wave, m, feats, col0, first, commit, final):
        """Frames first .. first + m - 1 from the tail and ``wave``; ``commit``: the push / flush ends with this launch (retain, advance)."""
        fe = self.frontend
        n = 0 if wave is None else wave.shape[1]
        tail_in, tail_out = self._turns(n, commit, final)
        new_first = self._tail_first if tail_out is None else retain_from(first + m, self.hop, self.win)
        rel = new_first - self._tail_first
        if m or tail_out is not None:
            hip.frontend_stream_step(tail_in, self._tail_len, self._tail_first, wave if n else None, tail_out, rel, self._dft_image,
                                     self._fbank_image, fe.mean, fe.inv_scale, feats, col0, first, m, final, self.win, self.hop, fe.bins)
        if commit:
            self.frames_out = first + m
            self._retained(n, tail_out, new_first)


class Resampler:
    """``resampler(wave, lengths=None) -> (resampled, out_lengths)``: (B, L) float32 samples at ``orig_freq`` on a HIP device to
    (B, ceil(n L / o)) samples at ``new_freq``, by band-limited sinc interpolation with a Hann window (the formula of DESIGN.md 9:
    torchaudio.functional.resample's defaults, written in absolute sample indices).  With ``lengths`` every utterance is resampled as
    if alone: nothing at or beyond its length is read and its outputs beyond ``out_len(length)`` are zero.  ``out_lengths``: a list.

    All arithmetic runs in libnbasr_hip.so (resample.hip); there is no CPU path.  Refused: rates that are not positive, and pairs whose
    reduced rates or support exceed the kernel's limits (``RESAMPLE_MAX_RATIO``, ``RESAMPLE_MAX_TAPS``)."""

    def __init__(self, orig_freq, new_freq=16000, device='cuda:0'):
        self.o, self.n = resample_ratio(orig_freq, new_freq)
        self.orig_freq, self.new_freq = int(orig_freq), int(new_freq)
        if max(self.o, self.n) > RESAMPLE_MAX_RATIO:
            raise ValueError(f'{orig_freq} -> {new_freq} reduces to {self.o} : {self.n}: the limit is {RESAMPLE_MAX_RATIO} on either side')
        self.taps = resample_taps(self.o, self.n)
        if self.taps > RESAMPLE_MAX_TAPS:
            raise ValueError(f'{orig_freq} -> {new_freq} has a support of {self.taps} taps: the limit is {RESAMPLE_MAX_TAPS}')
        self.device = torch.device(device)
        self.tail_capacity = resample_tail_capacity(self.o, self.n)
        self.max_pending = resample_max_pending(self.o, self.n)
        self.lookahead_samples = resample_lookahead(self.o, self.n)
        self._table = None

    def table(self):
        """The (n, taps | 1) coefficient table on the device: float64 on the host, rounded once to float32.  Made by the first use."""
        if self._table is None:
            self._table = torch.from_numpy(resample_table(self.o, self.n).astype(np.float32)).to(self.device).contiguous()
        return self._table

    def out_len(self, samples):
        return resample_total(int(samples), self.o, self.n)

    def stream(self, batch):
        """A ``ResamplerStream``: this resampler push by push for a lockstep batch of ``batch`` waveform streams."""
        return ResamplerStream(self, batch)

    def __call__(self, wave, lengths=None):
        if not isinstance(wave, torch.Tensor) or wave.dim() != 2 or wave.dtype != torch.float32 or not wave.is_cuda:
            raise hip.HipError('wave must be a (batch, samples) float32 tensor on a HIP device; this package has no CPU path')
        b, samples = wave.shape
        if samples and (wave.stride(1) != 1 or (b > 1 and wave.stride(0) < samples)):
            wave = wave.contiguous()
        out_lengths = [self.out_len(samples)] * b
        if lengths is not None:
            host = [int(v) for v in (lengths.tolist() if torch.is_tensor(lengths) else lengths)]
            if len(host) != b or min(host, default=0) < 0 or max(host, default=0) > samples:
                raise ValueError(f'lengths must be {b} values in [0, {samples}]')
            out_lengths = [self.out_len(v) for v in host]
            lengths = torch.tensor(host, dtype=torch.int32).to(wave.device)
        out = torch.empty(b, self.out_len(samples), device=wave.device)
        hip.resample(wave, lengths, self.table(), self.orig_freq, self.new_freq, out)
        return out, out_lengths


class ResamplerStream(_SampleTailStream):
    """``Resampler`` push by push (``Resampler.stream``): one HIP launch per push, state carried in two sample tails.

        rs = resampler.stream(batch=B)
        for chunk in waveform_chunks:              # (B, n) float32 on the device, any n >= 0
            y = rs.push(chunk)                     # (B, m): the outputs that are final now (resample_final)
        last = rs.flush()                          # (B, m): the outputs that needed the utterance's end
        # rs.peek() at any point before: the outputs flush() would return then, the stream left as it was
        # torch.cat([*pushes, last], 1) is resampler(whole waveform)[0]; the bits do not depend on the chunking

    ``FrontendStream``'s contract (both are ``_SampleTailStream``s): the batch is lockstep, ``flush`` twice or ``push`` after ``flush``
    raises.  ``state_bytes``: the two tails of ``resampler.tail_capacity`` samples per lane (the table belongs to the resampler)."""

    def __init__(self, resampler, batch):
        super().__init__(batch, resampler.device, resampler.tail_capacity)
        self.resampler = resampler
        self.o, self.n = resampler.o, resampler.n
        self.lookahead_samples = resampler.lookahead_samples
        self._table = resampler.table()
        assert self.state_bytes == hip.resample_state_bytes(self.batch, resampler.tail_capacity)
        self.reset()

    def reset(self):
        """Start the next batch of utterances; the tails are re-used."""
        super().reset()
        self.samples_out = 0

    @property
    def pending(self):
        """Outputs a flush or a peek would return now."""
        return resample_total(self.samples_in, self.o, self.n) - self.samples_out

    def push(self, wave_chunk):
        """Feed (batch, n) samples; returns the (batch, m) outputs that became final, m = resample_final(samples_in) - samples_out."""
        wave = self._admit(wave_chunk)
        m = resample_final(self.samples_in + wave.shape[1], self.o, self.n) - self.samples_out
        return self._step(wave, m, True, False)

    def flush(self):
        """End the utterance: its last outputs, with zeros beyond its end."""
        if self._flushed:
            raise ValueError('flush called twice: call reset() to start the next utterance')
        out = self._step(None, resample_total(self.samples_in, self.o, self.n) - self.samples_out, True, True)
        self._flushed = True
        return out

    def peek(self):
        """The outputs ``flush()`` would return now (``resample_peek``), with the stream left as it was."""
        if self._flushed:
            raise ValueError('peek after flush: call reset() to start the next utterance')
        return self._step(None, resample_total(self.samples_in, self.o, self.n) - self.samples_out, False, True)

    def _step(self, wave, m, commit, final):
        """Outputs samples_out .. samples_out + m - 1 from the tail and ``wave``; ``commit``: retain and advance."""
        r = self.resampler
        n = 0 if wave is None else wave.shape[1]
        out = torch.empty(self.batch, m, device=self.device)
        tail_in, tail_out = self._turns(n, commit, final)
        new_first = self._tail_first if tail_out is None else resample_retain_from(self.samples_out + m, self.o, self.n)
        rel = new_first - self._tail_first
        if m or tail_out is not None:
            hip.resample_stream_step(tail_in, self._tail_len, self._tail_first, wave if n else None, tail_out, rel, r.tail_capacity,
                                     self._table, r.orig_freq, r.new_freq, out, 0, self.samples_out, m, final)
        if commit:
            self.samples_out += m
            self._retained(n, tail_out, new_first)
        return out
