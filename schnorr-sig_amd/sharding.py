"""Batch-level sharding of a verification batch across the GPUs of one node.

The path shards by signature (each verification reads only its own (sig, pk, msg):
reference src/signature.rs:181-205), so there is no data-path collective.  The only
exchange is the aggregate verdict: one sum all-reduce of the per-rank rejection counts
(RCCL over xGMI on GPUs; gloo in the CPU tests), and an optional gather of status bytes.
"""


def shard_range(n, rank, world):
    """Contiguous range [lo, hi) of rank `rank`: sizes differ by at most one, earlier ranks larger."""
    if world <= 0 or not (0 <= rank < world):
        raise ValueError("bad rank/world")
    base, rem = divmod(n, world)
    lo = rank * base + min(rank, rem)
    return lo, lo + base + (1 if rank < rem else 0)


def aggregate_fail_count(local_count_tensor, dist=None):
    """In-place sum over ranks of a 1-element integer tensor; returns it. dist=None: single rank."""
    if dist is not None and dist.is_initialized() and dist.get_world_size() > 1:
        dist.all_reduce(local_count_tensor, op=dist.ReduceOp.SUM)
    return local_count_tensor


def batch_verdict(total_fail):
    """verify_batch's Result for the whole sharded batch (src/batch.rs:125-129): 0 Ok, 2 InvalidSignature."""
    return 0 if int(total_fail) == 0 else 2


def gather_status(local_status_tensor, n, rank, world, dist):
    """All-gather of per-shard status bytes into the full n-vector (ragged shards padded to the max)."""
    import torch
    if dist is None:
        return local_status_tensor
    width = (n + world - 1) // world
    pad = torch.full((width,), 255, dtype=local_status_tensor.dtype, device=local_status_tensor.device)
    pad[: local_status_tensor.numel()] = local_status_tensor
    parts = [torch.empty_like(pad) for _ in range(world)]
    dist.all_gather(parts, pad)
    out = []
    for r in range(world):
        lo, hi = shard_range(n, r, world)
        out.append(parts[r][: hi - lo])
    return torch.cat(out)


def scatter_rows(full, n, row_bytes, rank, world, dist, device=None, src=0):
    """Input distribution for a batch that is resident on rank `src`: every rank receives its own
    contiguous shard of the (n, row_bytes) uint8 array, each shard crossing one link once (direct
    scatter; a broadcast of the whole array would move `world` times the bytes and is ring/per-link
    bound on xGMI).  `full` is only read on rank `src`.  Equal shards are sent straight out of `full`
    (views, no staging copy); ragged shards are padded to the largest."""
    import torch
    lo, hi = shard_range(n, rank, world)
    if dist is None:        # no process group; with one the collective runs even at world size 1 (RCCL rehearsal)
        return full[lo:hi]
    width = (n + world - 1) // world
    dev = device if device is not None else (full.device if full is not None else "cpu")
    out = torch.empty((width, row_bytes), dtype=torch.uint8, device=dev)
    chunks = None
    if rank == src:
        if n % world == 0:
            chunks = [full[r * width:(r + 1) * width] for r in range(world)]
        else:
            chunks = []
            for r in range(world):
                a, b = shard_range(n, r, world)
                c = torch.zeros((width, row_bytes), dtype=torch.uint8, device=dev)
                c[: b - a] = full[a:b]
                chunks.append(c)
    dist.scatter(out, chunks, src=src)
    return out[: hi - lo]


def broadcast_rows(full, n, row_bytes, rank, world, dist, device=None, src=0):
    """The simpler distribution BASELINE.json's north_star names: broadcast the WHOLE (n, row_bytes) array
    from rank `src`, every rank then slices its own contiguous shard.  Moves `world` times the bytes of
    scatter_rows; kept as an option and timed beside it."""
    import torch
    lo, hi = shard_range(n, rank, world)
    if dist is None:
        return full[lo:hi]
    dev = device if device is not None else (full.device if full is not None else "cpu")
    buf = full if rank == src else torch.empty((n, row_bytes), dtype=torch.uint8, device=dev)
    dist.broadcast(buf, src=src)
    return buf[lo:hi]


MSM_PARTIAL_WORDS = 24   # SSA_MSM_PARTIAL_WORDS of include/schnorr_sig_amd.h


def gather_msm_partials(local_record, world, dist):
    """All-gather of the ranks' MSM-form shard records (int64[24] each, include/schnorr_sig_amd.h:
    ssa_verify_batch_msm_partial_device): 24 words per rank are the only traffic of the MSM-form verify_batch across
    processes (reference src/batch.rs:98-129: every shard contributes one point and one scalar).  Returns the
    (world, 24) tensor on every rank, in rank order; dist=None: the single record as a (1, 24) tensor."""
    import torch
    rec = local_record.reshape(MSM_PARTIAL_WORDS)
    if dist is None:
        return rec.reshape(1, MSM_PARTIAL_WORDS).clone()
    out = torch.empty(world * MSM_PARTIAL_WORDS, dtype=rec.dtype, device=rec.device)   # flat: gloo insists
    dist.all_gather_into_tensor(out, rec.contiguous())
    return out.reshape(world, MSM_PARTIAL_WORDS)


def msm_verdict(local_record, world, dist, combine, engine=None):
    """verify_batch's single verdict for a batch sharded over `world` ranks in the MSM form: gather the shard records,
    then `combine(records)` -- ssa_msm_combine[_device] on this rank's context: one point addition per shard, [sum]G,
    x-only compare -- on EVERY rank (each holds all the records, so no broadcast of the verdict is needed and the ranks
    cannot disagree: the combination is deterministic).  Returns (verdict, records).

    ORDERING.  ssa_verify_batch_msm_partial_device only ENQUEUES the record on the engine's stream, and the gather
    runs on torch's current stream: pass `engine` (the Engine that produced `local_record`) and the two are ordered
    here -- torch's stream waits for the engine before the gather (ssa_ctx_stream_release), the engine's stream waits
    for the gather before `combine` (ssa_ctx_stream_acquire), no host synchronisation.  With engine=None the caller
    vouches that the record is complete (Engine.sync(), or one shared stream through Engine.set_stream).  A record the
    kernel has not written yet is NOT mistaken for an empty shard: every record carries a magic word and the
    combination returns MALFORMED without it (include/schnorr_sig_amd.h)."""
    on_device = engine is not None and getattr(local_record, "is_cuda", False)
    if on_device:
        import torch
        engine.stream_release(torch.cuda.current_stream(local_record.device).cuda_stream)
    elif engine is not None:
        engine.sync()
    records = gather_msm_partials(local_record, world, dist)
    if on_device:
        engine.stream_acquire(torch.cuda.current_stream(local_record.device).cuda_stream)
    verdict = combine(records)
    if on_device:
        # torch's stream waits for the combination too: `records` (and the verdict buffer) may be released to torch's
        # caching allocator -- which reuses a block for later work on ITS stream -- while the engine's kernel still reads
        engine.stream_release(torch.cuda.current_stream(local_record.device).cuda_stream)
    return verdict, records


# ---- half-aggregation across ranks (include/schnorr_sig_amd.h "sharded half-aggregation") ----
def aggregate_block_range(n, block_lanes, rank, world):
    """Lanes [lo, hi) of rank `rank` when the ceil(n / block_lanes) blocks of an aggregate are dealt out whole:
    contiguous runs of blocks whose counts differ by at most one (shard_range over the blocks), the last block ragged."""
    if block_lanes <= 0 or block_lanes & (block_lanes - 1):
        raise ValueError("block_lanes must be a power of two")
    b_lo, b_hi = shard_range(-(-n // block_lanes), rank, world)
    return min(b_lo * block_lanes, n), min(b_hi * block_lanes, n)


def _engine_waits_for_torch(engine, t):
    """the engine's stream waits for what torch has queued (fresh buffers are filled on torch's stream)"""
    import torch
    if t.is_cuda:
        engine.stream_acquire(torch.cuda.current_stream(t.device).cuda_stream)


def _torch_waits_for_engine(engine, t):
    """torch's stream waits for the engine (msm_verdict's ORDERING); host tensors: a synchronisation"""
    import torch
    if t.is_cuda:
        engine.stream_release(torch.cuda.current_stream(t.device).cuda_stream)
    else:
        engine.sync()


def _gather_bytes(engine, local, world, dist):
    """All-gather of one equal-sized uint8 tensor per rank, ordered behind the engine's stream -> (world, len) on every
    rank, in rank order; dist=None: the single rank.  A gloo group gathers device tensors through host memory."""
    import torch
    _torch_waits_for_engine(engine, local)
    flat = local.reshape(-1).contiguous()
    if dist is None:
        return flat.reshape(1, -1).clone()
    through_host = flat.is_cuda and dist.get_backend() == "gloo"
    src = flat.cpu() if through_host else flat
    out = torch.empty(world * src.numel(), dtype=src.dtype, device=src.device)
    dist.all_gather_into_tensor(out, src)
    return (out.to(flat.device) if through_host else out).reshape(world, -1)


def _root_from_tops(engine, tops_local, n, block_lanes, world, dist):
    """the ranks' tops (each padded to the widest rank) gathered, trimmed and reduced to the root ON EVERY RANK, as
    msm_verdict lets every rank combine: 32 bytes per block are the traffic"""
    import torch
    gathered = _gather_bytes(engine, tops_local, world, dist)
    rows = []
    for r in range(world):
        lo, hi = aggregate_block_range(n, block_lanes, r, world)
        rows.append(gathered[r][: 32 * -(-(hi - lo) // block_lanes)])
    tops = torch.cat(rows).contiguous()
    root = torch.empty(32, dtype=torch.uint8, device=tops.device)
    _engine_waits_for_torch(engine, root)
    engine.aggregate_root_device(tops.data_ptr(), tops.numel() // 32, n, root.data_ptr(), block_lanes=block_lanes)
    return root, tops


def _shard_buffers(n, block_lanes, rank, world, like):
    import torch
    lo, hi = aggregate_block_range(n, block_lanes, rank, world)
    widest = -(-(-(-n // block_lanes)) // world)          # blocks of the widest rank
    return lo, hi, torch.zeros(max(widest, 1) * 32, dtype=torch.uint8, device=like.device)


def aggregate_sharded(engine, sigs, pks, msgs, n, block_lanes, rank=0, world=1, dist=None, pk_inf=None):
    """The producer over `world` ranks: this rank holds lanes aggregate_block_range(n, block_lanes, rank, world) of an
    aggregate of n as uint8 tensors on the engine's device (sigs (n_s, 81), pks (n_s, 96), dense msgs (n_s, len)).
    Returns (status, e_agg uint8[32], this rank's R's uint8[49 n_s], per-lane status uint8[n_s]): the aggregate is the
    ranks' R's in rank order and then e_agg, byte for byte Engine.aggregate of the whole batch; with a malformed lane
    anywhere status is 3 and e_agg is zero on every rank.  Two gathers: tops (32 bytes per block), partial scalars."""
    import torch
    lo, hi, tops_local = _shard_buffers(n, block_lanes, rank, world, sigs)
    n_s, dev = hi - lo, sigs.device
    e_part = torch.zeros(32, dtype=torch.uint8, device=dev)
    e_agg = torch.zeros(32, dtype=torch.uint8, device=dev)
    rs = torch.empty(49 * n_s, dtype=torch.uint8, device=dev)
    status = torch.zeros(n_s, dtype=torch.uint8, device=dev)
    nfail = torch.zeros(1, dtype=torch.int64, device=dev)
    inf = pk_inf.data_ptr() if pk_inf is not None and n_s else 0
    if n == 0:
        return 0, e_agg, rs, status
    _engine_waits_for_torch(engine, tops_local)
    if n_s:
        engine.aggregate_shard_tops_device(sigs.data_ptr(), 81, pks.data_ptr(), msgs.data_ptr(), n_s, msgs.shape[1],
                                           block_lanes, tops_local.data_ptr())
    root, _ = _root_from_tops(engine, tops_local, n, block_lanes, world, dist)
    engine.aggregate_shard_fold_device(sigs.data_ptr(), pks.data_ptr(), n_s, lo, root.data_ptr(), e_part.data_ptr(),
                                       rs.data_ptr(), d_status=status.data_ptr(), d_nfail=nfail.data_ptr(), d_pk_inf=inf)
    parts = _gather_bytes(engine, e_part, world, dist)
    total_fail = int(aggregate_fail_count(nfail.cpu() if dist is not None and dist.get_backend() == "gloo" else nfail,
                                          dist).item())
    if total_fail:
        return 3, e_agg, rs.zero_(), status
    _engine_waits_for_torch(engine, parts)
    engine.aggregate_combine_device(parts.data_ptr(), world, e_agg.data_ptr())
    _torch_waits_for_engine(engine, e_agg)
    return 0, e_agg, rs, status


def verify_aggregate_sharded(engine, rs49, pks, msgs, e_agg, n, block_lanes, rank=0, world=1, dist=None, pk_inf=None):
    """The validator over `world` ranks: this rank holds the R's (n_s, 49), keys and messages of its lanes
    (aggregate_block_range) and the aggregate's 32 bytes of e_agg, uint8 tensors on the engine's device.  Returns the
    status of Engine.verify_aggregate on the whole aggregate, on every rank.  Two gathers: tops, then one 24-word
    record per rank; every rank combines, and the combination fails closed as msm_verdict's does."""
    import torch
    lo, hi, tops_local = _shard_buffers(n, block_lanes, rank, world, pks)
    n_s, dev = hi - lo, pks.device
    h = torch.empty(32 * n_s, dtype=torch.uint8, device=dev)
    record = torch.zeros(MSM_PARTIAL_WORDS, dtype=torch.int64, device=dev)
    verdict = torch.full((1,), 3, dtype=torch.int32, device=dev)
    inf = pk_inf.data_ptr() if pk_inf is not None and n_s else 0
    _engine_waits_for_torch(engine, verdict)
    if n == 0:
        engine.verify_aggregate_combine_device(0, 0, e_agg.data_ptr(), 0, verdict.data_ptr())
    else:
        if n_s:
            engine.aggregate_shard_tops_device(rs49.data_ptr(), 49, pks.data_ptr(), msgs.data_ptr(), n_s, msgs.shape[1],
                                               block_lanes, tops_local.data_ptr(), d_h=h.data_ptr())
        root, _ = _root_from_tops(engine, tops_local, n, block_lanes, world, dist)
        engine.verify_aggregate_shard_device(rs49.data_ptr(), pks.data_ptr(), msgs.data_ptr(), n_s, msgs.shape[1],
                                             h.data_ptr(), lo, root.data_ptr(), record.data_ptr(), d_pk_inf=inf)
        records = _gather_bytes(engine, record.view(torch.uint8), world, dist)
        _engine_waits_for_torch(engine, records)
        engine.verify_aggregate_combine_device(records.data_ptr(), world, e_agg.data_ptr(), n, verdict.data_ptr())
    _torch_waits_for_engine(engine, verdict)
    return int(verdict.cpu().item())
