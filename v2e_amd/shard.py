"""One clip's SuperSloMo stage over the ranks of a process group: the frame side of multi-rank runs (`dist.py` is
the event-stream side).

The P = N - 1 source pairs of a clip are independent (slomo.py:330-466: every batch is computed from its own frames), so rank r
interpolates the contiguous block `pair_shard` gives it and the uint8 frames are assembled IN ORDER: on one rank, point to point
with exact sizes (`send_frames_to_owner_begin` / `_finish`), or on every rank by one all-gather of padded blocks
(`gather_frames_in_order`).  `run_chunked` takes a clip through in chunks, the owner's DVS stage on chunk c beside the ranks'
interpolation of chunk c + 1.  Block sizes follow from (pairs, world size) alone, so the ranks never exchange sizes.
"""
import torch
import torch.distributed as dist

from .planning import interp_frame_times
from .stream import join_chunks


def pair_shard(n_pairs, world, rank):
    """Source pairs [lo, hi) of rank `rank`: contiguous blocks r P / G .. (r + 1) P / G; empty when P < G leaves none."""
    return rank * n_pairs // world, (rank + 1) * n_pairs // world


def gather_frames_in_order(mine, n_pairs, U, group=None, owner=None):
    """The ranks' interpolated-frame blocks (uint8 [pairs_r U, H, W], pairs_r from pair_shard) in the clip's frame order.
    owner = a rank of the group: POINT TO POINT to that rank, exact sizes, received straight into the clip's tensor (round 6; an
    all-gather hands every rank the whole clip -- G - 1 times the receive volume anybody needs -- and wants the blocks padded to the
    largest); the other ranks return None.  owner = None: every rank assembles the clip (one all-gather of padded blocks).  Block
    sizes follow from (n_pairs, world) alone, so no size exchange is needed."""
    G, r = dist.get_world_size(group), dist.get_rank(group)
    cnt = [(pair_shard(n_pairs, G, q)[1] - pair_shard(n_pairs, G, q)[0]) * U for q in range(G)]
    assert int(mine.shape[0]) == cnt[r], "this rank interpolated %d frames, its shard has %d" % (int(mine.shape[0]), cnt[r])
    if owner is not None:
        reqs, clip = send_frames_to_owner_begin(n_pairs, U, tuple(mine.shape[1:]), mine, group, owner)
        for q in send_frames_to_owner_finish(reqs, clip, mine, n_pairs, U, group, owner):
            q.wait()
        return clip if r == owner else None
    m = max(cnt)
    pad = mine if cnt[r] == m else torch.cat((mine, mine.new_zeros((m - cnt[r],) + tuple(mine.shape[1:]))))
    parts = [torch.empty_like(pad) for _ in range(G)]
    dist.all_gather(parts, pad.contiguous(), group=group)
    return torch.cat([parts[q][:cnt[q]] for q in range(G)])


def _global_rank(group, q):
    return q if group is None or group is dist.group.WORLD else dist.get_global_rank(group, q)


def send_frames_to_owner_begin(n_pairs, U, frame_shape, like, group, owner):
    """Owner: the tensor of the n_pairs * U frames and one posted receive per other rank's block, straight into its slice (posted
    before the owner's own interpolation, so that a sender never waits for the receiver).  Other ranks: ([], None)."""
    G, r = dist.get_world_size(group), dist.get_rank(group)
    if r != owner:
        return [], None
    clip = like.new_empty((n_pairs * U,) + tuple(frame_shape))
    reqs = []
    for q in range(G):
        lo, hi = pair_shard(n_pairs, G, q)
        if q != owner and hi > lo:
            reqs.append(dist.irecv(clip[lo * U:hi * U], src=_global_rank(group, q), group=group))
    return reqs, clip


def send_frames_to_owner_finish(reqs, clip, mine, n_pairs, U, group, owner):
    """Owner: its own block copied into place, the receive requests handed back.  Other ranks: their block sent (a request to wait for)."""
    G, r = dist.get_world_size(group), dist.get_rank(group)
    lo, hi = pair_shard(n_pairs, G, r)
    if r == owner:
        if hi > lo:
            clip[lo * U:hi * U] = mine
        return reqs
    return [dist.isend(mine.contiguous(), dst=_global_rank(group, owner), group=group)] if hi > lo else []


def run_chunked(pipe, frames_u8, src_frame_interval_s, return_device, group, owner, chunk_pairs):
    """`VideoToEvents.run(group=, chunk_pairs=)`: the clip in chunks of chunk_pairs source pairs, every chunk sharded over the ranks
    and sent to the owner, whose DVS stage takes chunk c while the ranks, the owner included, interpolate chunk c + 1."""
    G, r = dist.get_world_size(group), dist.get_rank(group)
    N = int(frames_u8.shape[0])
    P, U = N - 1, pipe.U
    times = interp_frame_times(N, U, float(src_frame_interval_s), pipe.batch_size)
    shape = tuple(frames_u8.shape[1:])
    evs, counts, pending = [], [], None   # pending: (receive requests, the chunk's frames, its times) -- the chunk the owner takes next
    asynchronous = hasattr(pipe.emu, "generate_events_batch_async")
    runs = []

    def dvs(reqs, chunk, t):
        for q in reqs:
            q.wait()
        if asynchronous:  # enqueue; the result is read at the end (the emulator alternates two buffer sets: at most two in flight)
            runs.append(pipe.emu.generate_events_batch_async(chunk, t, return_device=return_device))
            while len(runs) > 1:
                e, c = runs.pop(0).result()
                # (device rows are a view of one of the emulator's two alternating buffers: the chunk after next overwrites it)
                evs.append(e.clone() if return_device and e is not None else e)
                counts.append(c)
        else:
            e, c = pipe.emu.generate_events_batch(chunk, t, return_device=return_device)
            evs.append(e)
            counts.append(c)

    for p0 in range(0, P, chunk_pairs):
        n = min(p0 + chunk_pairs, P) - p0
        # (the owner posts its receives BEFORE its own share of the interpolation: the other ranks' sends then complete as they finish)
        reqs, chunk = send_frames_to_owner_begin(n, U, shape, frames_u8, group, owner)
        lo, hi = pair_shard(n, G, r)
        mine = pipe.upsample(frames_u8[p0 + lo:p0 + hi + 1]) if hi > lo else frames_u8.new_empty((0,) + shape)
        if r == owner and pending is not None:  # the DVS stage of the chunk BEFORE, while this chunk's frames arrive
            dvs(*pending)
        reqs = send_frames_to_owner_finish(reqs, chunk, mine, n, U, group, owner)
        if r == owner:
            pending = (reqs, chunk, times[p0 * U:(p0 + n) * U])
        else:
            for q in reqs:
                q.wait()
    if r != owner:
        return None, None, P * U
    dvs(*pending)
    for run in runs:
        e, c = run.result()
        evs.append(e)
        counts.append(c)
    return join_chunks(evs, counts) + (P * U,)
