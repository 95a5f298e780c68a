"""Clip arithmetic of the SuperSloMo and video stages: which pairs go into which flow-UNet call, batch and chunk, the upsampling
factor of a batch, the time points of a factor, the sample table of a ragged chunk and the times of the interpolated frames.

Pure host planning on numpy (no torch, no library): `slomo.SuperSloMo`, `pipeline.VideoToEvents`, the streaming run and the
multi-rank frame path all take their numbers from here, so that a frame has one index and one time whichever of them made it.

Frame order and times follow slomo.py:391-400, 441 and v2e.py:786-797: output frame b*U + k of a batch has interpTime
pair + k/U (in source frame intervals), and v2e.py stretches the interpTimes so that they SPAN the processed duration of the
source clip: t = interpTime * (N_src - 1) * interval / (max(interpTimes) - min(interpTimes)).
"""
import numpy as np


def speed_from_bits(bits):
    """The flow speed (pixels per source frame) from the float32 bits of a squared-speed maximum (v2e_slomo_max_speed2): ONE
    float32 sqrt, as slomo.py:359-368 takes it per plane; NaN for the NaN marker 0xffffffff."""
    bits = int(bits) & 0xFFFFFFFF
    if bits == 0xFFFFFFFF:
        return float("nan")
    return float(np.sqrt(np.array([bits], dtype=np.uint32).view(np.float32)[0]))


def factor_from_speed(speed, minimum=None):
    """slomo.py:352-379: a batch's upsampling factor from its largest flow speed: the ceil, at least `minimum` (None: no minimum)
    and at least 2.  A NaN flow raises ValueError, as int(np.ceil(nan)) does in the reference."""
    if speed != speed:
        raise ValueError("auto_upsample: the flow of a batch is NaN, so its upsampling factor is undefined")
    u = int(np.ceil(speed))
    if minimum is not None and minimum > u:
        u = minimum
    if u < 2:
        u = 2
    return u


def auto_upsampling_factor(speed_bits, minimum=None):
    """`factor_from_speed` of the float32 bits of a batch's largest squared flow speed (v2e_slomo_max_speed2)."""
    return factor_from_speed(speed_from_bits(speed_bits), minimum)


def time_points(u):
    """slomo.py:405: the time points (k + 0.5) / u of upsampling factor u within a source frame interval, as Python floats."""
    return [(k + 0.5) / u for k in range(u)]


def time_coefficients(ts):
    """[n_t][6] float32: fCoeff[0..3] (slomo.py:406-407) and wCoeff (:429), in Python doubles first."""
    rows = []
    for t in ts:
        t = float(t)
        temp = -t * (1 - t)
        rows.append([temp, t * t, (1 - t) * (1 - t), temp, 1 - t, t])
    return np.asarray(rows, dtype=np.float64).astype(np.float32)


def interp_times(n_src, U, batch_size=None, factors=None):
    """The un-normalised interpTimes of slomo.interpolate (slomo.py:388-400): per batch of `batch_size` pairs (None: one batch)
    inputFrameCounter + k * (1 / U_b), k < U_b * pairs in the batch.  factors: U_b per batch (auto_upsample); None: U for all."""
    npairs = n_src - 1
    bs = npairs if not batch_size else int(batch_size)
    starts = range(0, npairs, bs)
    factors = [U] * len(starts) if factors is None else [int(u) for u in factors]
    if len(factors) != len(starts):
        raise ValueError("%d upsampling factors for %d batches" % (len(factors), len(starts)))
    return np.concatenate([_batch_interp_times(b0, u, min(bs, npairs - b0)) for b0, u in zip(starts, factors)])


def _batch_interp_times(b0, u, nb):
    """The interpTimes of one batch of nb pairs starting at pair b0 with factor u (slomo.py:393-398)."""
    return b0 + np.array(range(u * nb)) * (1 / u)


def interp_frame_times(n_src, U, src_frame_interval_s, batch_size=None, factors=None):
    """Times of the interpolated frames as v2e.py computes them, operation for operation: interpTimes are built per batch of
    `batch_size` pairs as inputFrameCounter + k * (1 / U) (`interp_times`; factors: one U per batch, auto_upsample), then
    normalised to the processed duration of the source clip (v2e.py:786-797: f = srcVideoRealProcessedDuration / (max(interpTimes) -
    min(interpTimes)); interpTimes = f * interpTimes)."""
    interp = interp_times(n_src, U, batch_size, factors)
    duration = (n_src - 1) * float(src_frame_interval_s)
    f = duration / (np.max(interp) - np.min(interp))
    return f * interp


def auto_sample_table(factors, n_pairs, batch_size):
    """The samples of a flow chunk of n_pairs pairs whose batches of batch_size pairs have the upsampling factors `factors`, in v2e
    frame order (slomo.py:441: batch offset + U_b * pair in batch + k): (ts, tab, cuts) with ts the `time_points` of every
    distinct U, tab one (pair, row of ts, output frame) per sample, cuts the batches' first samples and the end.  Every entry is
    checked against the sizes: the kernels index with them."""
    if (len(factors) - 1) * batch_size >= n_pairs or len(factors) * batch_size < n_pairs:
        raise ValueError("%d factors for %d pairs in batches of %d" % (len(factors), n_pairs, batch_size))
    ts, row0 = [], {}
    for u in sorted(set(factors)):
        row0[u] = len(ts)
        ts += time_points(u)
    tab, cuts = [], [0]
    for j, u in enumerate(factors):
        b0, b1 = j * batch_size, min((j + 1) * batch_size, n_pairs)
        for i in range(b0, b1):
            for k in range(u):
                tab.append((i, row0[u] + k, cuts[-1] + u * (i - b0) + k))
        cuts.append(len(tab))
    n = len(tab)
    assert all(0 <= p < n_pairs and 0 <= r < len(ts) and 0 <= f < n for p, r, f in tab)
    return ts, tab, cuts


def flow_chunk_pairs(batch_size):
    """Pairs per flow-UNet call of `upsample`: whole interpolation batches, as many as fit in 64 pairs (one at least).  The flow
    UNet's small levels fill the GPU only with many samples, and a pair's flow does not depend on what else is in the batch."""
    return int(batch_size) * max(1, 64 // int(batch_size))


def flow_chunks(n_pairs, batch_size):
    """The pairs [(f0, f1)] of every flow-UNet call of `upsample` on n_pairs pairs, fixed and automatic factors alike."""
    fc, n_pairs = flow_chunk_pairs(batch_size), int(n_pairs)
    return [(f0, min(f0 + fc, n_pairs)) for f0 in range(0, n_pairs, fc)]


def last_flow_chunk(n_pairs, batch_size):
    """The pairs (f0, n_pairs) of the clip's last flow-UNet call in `upsample`."""
    return flow_chunks(n_pairs, batch_size)[-1]


def stream_chunks(n_pairs, batch_size, chunk_pairs=None):
    """The chunks [(p0, p1)] of source pairs that `VideoToEvents.run_stream` takes in turn.  chunk_pairs must be a positive multiple
    of the flow chunk (`flow_chunk_pairs`; default four of them): every flow-UNet call, interpolation call and auto_upsample sample
    packing of a chunk is then the very call the unchunked `upsample` makes, which keeps the frames bit-identical under the conv maths
    that scale activations per call.  A clip shorter than one chunk is one chunk."""
    fc = flow_chunk_pairs(batch_size)
    if chunk_pairs is None:
        chunk_pairs = 4 * fc
    if isinstance(chunk_pairs, bool) or int(chunk_pairs) != chunk_pairs or chunk_pairs <= 0 or int(chunk_pairs) % fc:
        raise ValueError("chunk_pairs must be a positive multiple of the flow chunk of %d pairs (batch_size %d), got %r"
                         % (fc, int(batch_size), chunk_pairs))
    chunk_pairs, n_pairs = int(chunk_pairs), int(n_pairs)
    return [(p0, min(p0 + chunk_pairs, n_pairs)) for p0 in range(0, n_pairs, chunk_pairs)]


def stream_time_scale(n_src, src_frame_interval_s, batch_size, last_factor):
    """The factor f of `interp_frame_times` (v2e.py:786-797: processed duration / (max(interpTimes) - min(interpTimes))) from the
    factor of the clip's LAST batch alone: interpTimes rise batch after batch, so the maximum is the last batch's last time, the
    minimum the first batch's first, 0."""
    npairs = int(n_src) - 1
    bs = int(batch_size)
    b0 = (npairs - 1) // bs * bs
    last = _batch_interp_times(b0, int(last_factor), npairs - b0)
    duration = npairs * float(src_frame_interval_s)
    return duration / (np.max(last) - 0.0)


def chunk_frame_times(p0, p1, batch_size, factors, scale):
    """Times of the interpolated frames of source pairs [p0, p1) (p0 a multiple of batch_size), `factors` the U of each of their
    batches: the slice of `interp_frame_times` for the whole clip that belongs to them, bit for bit (`scale`: stream_time_scale)."""
    bs = int(batch_size)
    starts = range(p0, p1, bs)
    if p0 % bs or len(factors) != len(starts):
        raise ValueError("%d factors for pairs [%d, %d) in batches of %d" % (len(factors), p0, p1, bs))
    parts = [_batch_interp_times(b0, int(u), min(bs, p1 - b0)) for b0, u in zip(starts, factors)]
    return scale * np.concatenate(parts)
