"""Multi-GPU sharding of the hot path, one process per GPU over torch.distributed
(backend "nccl" == RCCL over xGMI on the MI355X node; "gloo" in the CPU tests).

Two regimes:

* independent units -- frames of motion's default `-b 0x0x1` (motion/motion.c:174,613-615), channel
  planes or whole images: `shard_range()` gives each rank a contiguous range; NO collective on the
  data path (bench.py uses this: weak scaling).

* one 3-D block spanning the whole clip (`-b 0x0x0`, motion/motion.c:535-552: REDFT10^3 / REDFT01^3 on a
  {d,h,w} block): `SlabDCT3D`.  Each rank owns a block of consecutive frames.  Forward = local y and x
  passes -> all-to-all that re-slabs the volume by rows (each rank then owns a block of rows of ALL
  frames) -> local z pass.  The coefficients stay in the z-local layout, where motion's filters
  (elementwise, motion.c:650-744) can run; inverse = z pass -> all-to-all back -> x and y passes.
  The x pass writes / reads the exchange buffers itself (no pack or unpack sweep), the exchange is cut into
  pieces that overlap the neighbouring pieces' passes, and d, h need not divide by the number of ranks.
  No all-reduce anywhere; xGMI is point-to-point and an all-to-all uses all 7 links at once.
"""
import math

import torch
import torch.distributed as dist

from .engine import Plan, REDFT01, REDFT10


def shard_range(n, rank, world):
    """contiguous [lo, hi) of n independent units for `rank` (sizes differ by at most one)"""
    base, rem = divmod(n, world)
    lo = rank * base + min(rank, rem)
    return lo, lo + base + (1 if rank < rem else 0)


def block_range(n, rank, world):
    """[lo, hi) of rank's block when n units are dealt in EQUAL blocks of ceil(n / world) (the last blocks may be short or
    empty): the layout SlabDCT3D uses for frames and for rows, because equal blocks make every exchange buffer an affine
    array (no gaps to pack around) whatever n % world is"""
    per = -(-n // world)
    return min(n, rank * per), min(n, (rank + 1) * per)


class SlabDCT3D:
    """Distributed 3-D DCT-II / DCT-III of a {d,h,w} f32 volume (motion -b 0x0x0, motion/motion.c:535-552,641,753), slab-decomposed
    over the ranks of `group`.  `uniform=True` fuses motion's uniform-range scaling (motion.c:644-647 forward, :748-751 inverse)
    into the passes; the inverse additionally applies 1/(8 d h w).

    Layout.  Rank r owns frames block_range(d, r, G) of the clip ([dl, h, w], all rows) before the forward transform and rows
    block_range(h, r, G) of the coefficients afterwards ([d, hl, w], all frames).  d and h need NOT divide by G (BASELINE config 5's
    chroma planes are 960 x 540: 540 = 7 x 68 + 64 on 8 ranks): blocks are ceil-sized, the last one short.

    No pack / unpack sweeps.  The x pass is the LAST local pass of the forward transform and the FIRST after the inverse
    exchange, and it is separable by lines, so it writes (reads) the exchange buffers directly through its batch strides:
      forward   y pass in place on [dl, h, w]  ->  x pass of rows [r*hp + c0, ...) of every frame, straight into
                send[r] = [dlp, ch, w]  ->  all_to_all_single  ->  recv = [G*dlp, ch, w] = every frame, my rows  ->  z pass from
                recv (frame stride ch*w) into coeffs [d, hl, w]
      inverse   z pass from coeffs into send = [G*dlp, ch, w]  ->  all_to_all_single  ->  x pass from recv[s] = [dlp, ch, w]
                straight into rows [s*hp + c0, ...) of [dl, h, w]  ->  y pass in place
    Pipelined: the rows of a block are cut into `chunks` pieces; the exchange of piece p (RCCL, its own stream) runs while the x pass
    of piece p+1 and the z pass of piece p-1 run on the compute stream.  Two all-to-alls per roundtrip, no all-reduce; xGMI is
    point-to-point and an all-to-all uses all 7 links at once."""

    def __init__(self, d, h, w, group=None, uniform=True, lib=None, chunks=None):
        self.group = group
        self.G = dist.get_world_size(group) if dist.is_initialized() else 1
        self.rank = dist.get_rank(group) if dist.is_initialized() else 0
        G = self.G
        self.d, self.h, self.w = d, h, w
        self.dlp, self.hp = -(-d // G), -(-h // G)               # block sizes (frames, rows)
        self.f_lo, self.f_hi = block_range(d, self.rank, G)
        self.y_lo, self.y_hi = block_range(h, self.rank, G)
        self.dl, self.hl = self.f_hi - self.f_lo, self.y_hi - self.y_lo
        if chunks is None:
            chunks = 1 if G == 1 else 4
        self.ch = -(-self.hp // max(1, min(chunks, self.hp)))    # rows per piece
        self.P = -(-self.hp // self.ch)
        self.lib = lib
        self.uniform = uniform
        self._plans = {}
        self._bufs = {}
        r2 = math.sqrt(2.0)
        u = (lambda p, fwd: p.set_axis_scale0(0, 1.0, 1.0 / r2) if fwd else p.set_axis_scale0(0, r2, 1.0)) if uniform else (lambda p, fwd: p)
        self._u = u
        dl, hl = self.dl, self.hl
        # y pass, in place on my frames: transform dim (h, stride w), batch (w, 1) x (dl, h*w)
        self.fwd_y = self.inv_y = None
        if dl:
            self.fwd_y = u(Plan.guru([(h, w, w)], [(w, 1, 1), (dl, h * w, h * w)], [REDFT10], lib=lib), True)
            self.inv_y = u(Plan.guru([(h, w, w)], [(w, 1, 1), (dl, h * w, h * w)], [REDFT01], lib=lib), False).set_scale(1.0 / (8.0 * d * h * w))

    # ---- plans that depend on a piece's row count (cached: at most three distinct counts occur) ----
    def _plan_x(self, nrows, fwd, nblocks=1):
        """x pass over `nrows` rows of every one of my frames, for `nblocks` consecutive destination (source) ranks in ONE launch: between
        the frame layout [dl, h, w] (the blocks' rows hp rows apart) and the blocks [dlp, ch, w] of an exchange buffer (dlp*ch*w apart).
        Round 3 launched one execution per rank: at 8 ranks x 4 pieces 32 launches of ~34 rows x 32 frames per plane and direction,
        launch-bound before xGMI is; the third batch level of the row passes (PassGeom::sb2_*) makes it one per piece."""
        key = ("x", nrows, fwd, nblocks)
        if key not in self._plans:
            w, h, ch = self.w, self.h, self.ch
            img, blk = (nblocks, self.hp * w), (nblocks, self.dlp * ch * w)
            if fwd:
                dims = [(nrows, w, w), (self.dl, h * w, ch * w)] + ([(img[0], img[1], blk[1])] if nblocks > 1 else [])
                p = Plan.guru([(w, 1, 1)], dims, [REDFT10], lib=self.lib)
            else:
                dims = [(nrows, w, w), (self.dl, ch * w, h * w)] + ([(img[0], blk[1], img[1])] if nblocks > 1 else [])
                p = Plan.guru([(w, 1, 1)], dims, [REDFT01], lib=self.lib)
            self._plans[key] = self._u(p, fwd)
        return self._plans[key]

    def _groups(self, p):
        """runs of consecutive blocks whose piece p has the same number of rows: [(first block, blocks, rows)] -- all full blocks form
        one run, a short last block its own, empty blocks none: at most two x-pass launches per piece whatever G is"""
        out = []
        for r in range(self.G):
            y0, y1 = self._rows_of(r, p)
            n = y1 - y0
            if n <= 0:
                continue
            if out and out[-1][2] == n and out[-1][0] + out[-1][1] == r:
                out[-1] = (out[-1][0], out[-1][1] + 1, n)
            else:
                out.append((r, 1, n))
        return out

    def _plan_z(self, nrows, fwd):
        """z pass over the columns of `nrows` of my rows, between a received piece [G*dlp, ch, w] and coeffs [d, hl, w]"""
        key = ("z", nrows, fwd)
        if key not in self._plans:
            w, ch, hl, d = self.w, self.ch, self.hl, self.d
            r2 = math.sqrt(2.0)
            if fwd:
                p = Plan.guru([(d, ch * w, hl * w)], [(nrows * w, 1, 1)], [REDFT10], lib=self.lib)
                p = self._u(p, True)
                if self.uniform:
                    p.set_scale(2.0 * r2)
            else:
                p = Plan.guru([(d, hl * w, ch * w)], [(nrows * w, 1, 1)], [REDFT01], lib=self.lib)
                p = self._u(p, False)
                if self.uniform:
                    p.set_scale(1.0 / (2.0 * r2))
            self._plans[key] = p
        return self._plans[key]

    def _buf(self, name, like):
        n = self.P * self.G * self.dlp * self.ch * self.w
        b = self._bufs.get(name)
        if b is None or b.device != like.device:
            b = torch.zeros(n, dtype=torch.float32, device=like.device)
            self._bufs[name] = b
        return b.view(self.P, self.G, self.dlp, self.ch, self.w)

    @staticmethod
    def _stream(t):
        return torch.cuda.current_stream(t.device).cuda_stream if t.is_cuda else 0

    def _rows_of(self, r, p):
        """image rows of block r that fall into piece p: [y0, y1)"""
        lo, hi = block_range(self.h, r, self.G)
        y0 = min(hi, lo + p * self.ch)
        return y0, min(hi, y0 + self.ch)

    def _exchange(self, send, recv):
        if self.G == 1:
            return None                             # one rank: forward() / inverse() alias recv to send
        return dist.all_to_all_single(recv.view(-1), send.view(-1), group=self.group, async_op=True)

    def exchange_alone(self, like):
        """the P all-to-alls of one forward() (equally of one inverse()) with no pass beside them and each waited for: what the bench derives the
        exchange time and the xGMI fraction from.  `like`: any tensor on this rank's device.  Returns the bytes this rank sends to
        OTHER ranks in them (its own piece of every all-to-all stays local)."""
        send = self._buf("send", like)
        recv = send if self.G == 1 else self._buf("recv", like)
        for p in range(self.P):
            w = self._exchange(send[p], recv[p])
            if w is not None:
                w.wait()
        return send.numel() * 4 * (self.G - 1) // self.G

    def forward(self, frames):
        """frames: [dl, h, w] f32 (this rank's frames, block_range(d, rank, G); overwritten).  Returns [d, hl, w] coefficients of
        REDFT10^3 (uniform range if requested) for this rank's rows block_range(h, rank, G)."""
        assert tuple(frames.shape) == (self.dl, self.h, self.w) and frames.dtype == torch.float32 and frames.is_contiguous()
        st = self._stream(frames)
        send = self._buf("send", frames)
        recv = send if self.G == 1 else self._buf("recv", frames)
        coeffs = torch.empty((self.d, self.hl, self.w), dtype=torch.float32, device=frames.device)
        if self.dl:
            self.fwd_y.execute(frames.data_ptr(), stream=st)
        es = 4
        work = [None] * self.P

        def zpass(p):
            if work[p] is not None:
                work[p].wait()                      # RCCL: the compute stream waits for the collective; gloo: the host does
            y0, y1 = self._rows_of(self.rank, p)
            if y1 > y0:
                self._plan_z(y1 - y0, True).execute(recv[p].data_ptr(), coeffs.data_ptr() + (y0 - self.y_lo) * self.w * es, stream=st)

        for p in range(self.P):
            for r0, nb, n in (self._groups(p) if self.dl else []):
                y0 = self._rows_of(r0, p)[0]
                self._plan_x(n, True, nb).execute(frames.data_ptr() + y0 * self.w * es, send[p, r0].data_ptr(), stream=st)
            work[p] = self._exchange(send[p], recv[p])
            if p > 0:
                zpass(p - 1)
        zpass(self.P - 1)
        return coeffs

    def inverse(self, coeffs):
        """coeffs: [d, hl, w] (this rank's rows; not modified).  Returns this rank's [dl, h, w] frames, scaled by 1/(8dhw)."""
        assert tuple(coeffs.shape) == (self.d, self.hl, self.w) and coeffs.is_contiguous()
        st = self._stream(coeffs)
        send = self._buf("send", coeffs)
        recv = send if self.G == 1 else self._buf("recv", coeffs)
        frames = torch.empty((self.dl, self.h, self.w), dtype=torch.float32, device=coeffs.device)
        es = 4
        work = [None] * self.P

        def xpass(p):
            if work[p] is not None:
                work[p].wait()
            for s0, nb, n in (self._groups(p) if self.dl else []):
                y0 = self._rows_of(s0, p)[0]
                self._plan_x(n, False, nb).execute(recv[p, s0].data_ptr(), frames.data_ptr() + y0 * self.w * es, stream=st)

        for p in range(self.P):
            y0, y1 = self._rows_of(self.rank, p)
            if y1 > y0:
                self._plan_z(y1 - y0, False).execute(coeffs.data_ptr() + (y0 - self.y_lo) * self.w * es, send[p].data_ptr(), stream=st)
            work[p] = self._exchange(send[p], recv[p])
            if p > 0:
                xpass(p - 1)
        xpass(self.P - 1)
        if self.dl:
            self.inv_y.execute(frames.data_ptr(), stream=st)
        return frames


class ChannelShardedScan:
    """BASELINE config 4's multi-GPU layout: scan's progressive reconstruction (scan/scan.c:292-298,377-383,421-459)
    with the colour planes of the interleaved image spread over the ranks (plane z on rank z % G; a rank may own
    several planes or none).  Planes are independent, so there is NO collective in the frame loop; `gather()` uses
    one all_gather to rebuild the interleaved sum on every rank (e.g. to encode the output frame).

    Each rank holds its planes planar ([h][w] f32): forward REDFT10^2 with the 1/(4wh) normalisation fused, zigzag
    frame ids, then per output frame one fused masked-accumulate execution (or the pruned path for tiny steps).
    A rank that owns EVERY plane (one GPU) keeps the image interleaved as the tool has it (scan.c:292-293) and runs one
    execution per frame for the three channels instead of three; `layout="planar"` forces the planar form there too."""

    def __init__(self, image_hwc, step, group=None, lib=None, layout="auto"):
        from . import _lib
        self.lib = lib or _lib.load()
        self.group = group
        self.G = dist.get_world_size(group) if dist.is_initialized() else 1
        self.rank = dist.get_rank(group) if dist.is_initialized() else 0
        self.h, self.w, self.c = image_hwc.shape
        self.step = int(step)
        self.nframes = (self.w * self.h + self.step - 1) // self.step          # scan.c:347-348 with limit = w*h
        self.mine = [z for z in range(self.c) if z % self.G == self.rank]
        if layout not in ("auto", "planar"):
            raise ValueError("layout is 'auto' or 'planar'")
        self.interleaved = layout == "auto" and len(self.mine) == self.c
        self.nch = self.c if self.interleaved else 1             # channels of one execution
        dev = image_hwc.device
        if self.interleaved:
            self.coeffs = [image_hwc.contiguous().clone()]
            self.fwd = Plan.image(self.h, self.w, self.c, REDFT10, lib=lib).set_scale(1.0 / (4.0 * self.w * self.h))
            self.inv = Plan.image(self.h, self.w, self.c, REDFT01, lib=lib)
        else:
            self.coeffs = [image_hwc[:, :, z].contiguous().clone() for z in self.mine]
            self.fwd = Plan.many_r2r([self.h, self.w], [REDFT10] * 2, lib=lib).set_scale(1.0 / (4.0 * self.w * self.h))
            self.inv = Plan.many_r2r([self.h, self.w], [REDFT01] * 2, lib=lib)
        self.ids = torch.zeros(self.w * self.h, dtype=torch.int32, device=dev)
        st = SlabDCT3D._stream(image_hwc) or None     # every helper on torch's current stream, like the transforms
        self._check(self.lib.dspfft_scan_zigzag_frame_ids(self.ids.data_ptr(), self.w, self.h, self.step, st))
        # the owner ids stay the same over the frames: let the fused step skip the column tiles a frame does not touch without reading their ids
        self.inv.scan_prepare(self.ids.data_ptr(), self.nch, stream=st or 0)
        self.work = torch.empty_like(self.coeffs[0]) if self.coeffs else None
        self.sums = []
        for cz in self.coeffs:
            self.fwd.execute(cz.data_ptr(), stream=SlabDCT3D._stream(cz))
            s = torch.empty_like(cz)
            self._check(self.lib.dspfft_broadcast_dc(s.data_ptr(), cz.data_ptr(), self.w * self.h, self.nch, st))   # scan.c:377-383
            self.sums.append(s)
        self.frame = 0

    def _check(self, rc):
        if rc:
            raise RuntimeError(self.lib.dspfft_last_error().decode())

    def warm(self):
        """one step with a frame id that no coefficient carries: every column tile is skipped and zeros are added to the running sums, which
        stay as they are -- loads the step's kernels before a timed loop"""
        for cz, s in zip(self.coeffs, self.sums):
            self.inv.execute_masked_accumulate(cz.data_ptr(), self.work.data_ptr(), s.data_ptr(), self.ids.data_ptr(), self.nframes, self.nch,
                                               stream=SlabDCT3D._stream(cz))

    def next_frame(self):
        """adds the coefficients of output frame `self.frame` into this rank's running sums"""
        if self.frame >= self.nframes:
            return False
        for cz, s in zip(self.coeffs, self.sums):
            self.inv.execute_masked_accumulate(cz.data_ptr(), self.work.data_ptr(), s.data_ptr(), self.ids.data_ptr(), self.frame, self.nch,
                                               stream=SlabDCT3D._stream(cz))
        self.frame += 1
        return True

    def gather(self):
        """interleaved (h, w, c) running sum on every rank"""
        dev = self.ids.device
        if self.interleaved:
            return self.sums[0].clone()
        out = torch.empty((self.h, self.w, self.c), dtype=torch.float32, device=dev)
        if self.G == 1:
            for z, s in zip(self.mine, self.sums):
                out[:, :, z] = s
            return out
        per = (self.c + self.G - 1) // self.G
        send = torch.zeros((per, self.h, self.w), dtype=torch.float32, device=dev)
        for i, s in enumerate(self.sums):
            send[i] = s
        recv = [torch.empty_like(send) for _ in range(self.G)]
        dist.all_gather(recv, send, group=self.group)
        for z in range(self.c):
            out[:, :, z] = recv[z % self.G][z // self.G]
        return out


#: scan method names in the numbering of include/dspfft.h (DSPFFT_SCAN_*)
SCAN_METHODS = ["horizontal", "vertical", "zigzag", "row", "column", "diagonal", "mirror", "box", "ibox", "radial", "iradial"]
_NONE = 0xFFFFFFFF


class FrameShardedScan:
    """scan's progressive reconstruction (scan/scan.c:346-459) with the OUTPUT FRAMES spread over the ranks, the four frame-loop options
    included: offset (-O, with the fill of :389-417 unless fill=False, i.e. --skip), invert (-I) and nframes (-n).

    The step is linear -- sum_k = sum_{k-1} + D3(c * mask_k) -- so a rank that owns frames [f0, f1) starts from the DC broadcast + the fill
    + ONE range-masked inverse (dspfft_execute_masked_accumulate_range) over every scan index the loop adds before f0, and then runs its own
    frames with the fused step: no collective anywhere.  Every rank holds the whole interleaved image (its own forward, 1/(4wh) fused).
    The loop frames [offset, offset + nframes) are dealt in contiguous ranges whose sizes differ by at most one (shard_range: equal
    blocks would leave the last ranks empty, e.g. 2, 2, 1, 0 frames for 5 on 4 ranks); with G ranks a rank runs at most
    ceil(nframes / G) + 1 step-equivalents, so the ceiling of the speed-up is nframes / (ceil(nframes / G) + 1): 3.56x for 32 frames
    on 4 GPUs, 6.4x on 8, against 3.0x for ChannelShardedScan, which leaves ranks beyond the colour planes idle.  G = 1 is the
    single-GPU device scan with those options.

    Frames come out on their owner only.  A caller who needs them in order collects frame i from owner(i): e.g. every rank runs its
    next_frame() in lock step and then, for the frame of each rank, dist.broadcast(sum, src=owner(i)) into a buffer of its own.

    Reference arithmetic kept as it is (scan.c:347-348,385-386,389-424): nframes = 0 or > limit/step becomes ceil(limit/step); offset >= limit
    becomes limit - 1; the fill adds scan indices [0, offset) (inverted: [limit - offset, limit)) while the loop starts at FRAME offset, i.e.
    scan index offset * step, so with step > 1 indices [offset, offset * step) are never added; frames past limit add nothing.
    Methods: every one dspfft_scan_frame_ids takes (box has no owner index: host/scan_dev stamps its frames instead)."""

    def __init__(self, image_hwc, step, method="zigzag", offset=0, fill=True, invert=False, nframes=0, group=None, lib=None):
        from . import _lib
        if method == "box":
            raise ValueError("FrameShardedScan: box has no owner index (a pixel can belong to several scan indices); host/scan_dev runs it by stamps")
        if method not in SCAN_METHODS:
            raise ValueError(f"FrameShardedScan: unknown scan method {method!r}")
        self.lib = lib or _lib.load()
        self.group = group
        self.G = dist.get_world_size(group) if dist.is_initialized() else 1
        self.rank = dist.get_rank(group) if dist.is_initialized() else 0
        self.h, self.w, self.c = image_hwc.shape
        self.step = int(step)
        if self.step < 1:
            raise ValueError("step must be >= 1")
        self.method = SCAN_METHODS.index(method)
        self.invert, self.fill = bool(invert), bool(fill)
        self.limit = int(self.lib.dspfft_scan_limit(self.method, self.w, self.h))
        nframes = int(nframes)
        if not nframes or nframes > self.limit // self.step:                    # scan.c:347-348
            nframes = (self.limit + self.step - 1) // self.step
        self.nframes = nframes
        self.offset = min(int(offset), self.limit - 1)                          # scan.c:385-386
        lo, hi = shard_range(self.nframes, self.rank, self.G)
        self.f0, self.f1 = self.offset + lo, self.offset + hi
        self._st = SlabDCT3D._stream(image_hwc) or None
        self.coeffs = image_hwc.contiguous().clone()
        fwd = Plan.image(self.h, self.w, self.c, REDFT10, lib=lib).set_scale(1.0 / (4.0 * self.w * self.h))
        fwd.execute(self.coeffs.data_ptr(), stream=self._st or 0)
        self.inv = Plan.image(self.h, self.w, self.c, REDFT01, lib=lib)
        dev = image_hwc.device
        # the owner index with DC unmarked (scan.c:406,445 clear it before every inverse): the fill, the prefix and every inverted frame
        self.index = torch.empty(self.w * self.h, dtype=torch.int32, device=dev)
        self._check(self.lib.dspfft_scan_owner_index(self.index.data_ptr(), self.method, self.w, self.h, self._st))
        self.index[0] = -1
        # forward frames: the frame ids of the single-GPU loop, prepared (tile ranges, element-id table) as ChannelShardedScan does
        self.ids = None
        if not self.invert:
            self.ids = torch.empty(self.w * self.h, dtype=torch.int32, device=dev)
            self._check(self.lib.dspfft_scan_frame_ids(self.ids.data_ptr(), self.method, self.w, self.h, self.step, self._st))
        self.inv.scan_prepare((self.index if self.invert else self.ids).data_ptr(), self.c, stream=self._st or 0)
        self.work = torch.empty_like(self.coeffs)
        self.sum = torch.empty_like(self.coeffs)
        self.start()

    def _check(self, rc):
        if rc:
            raise RuntimeError(self.lib.dspfft_last_error().decode())

    def _mirror(self, lo, hi):
        """scan indices [lo, hi) of the loop's order as owner indices: themselves, or limit - 1 - s when inverted (scan.c:391,424)"""
        lo, hi = min(lo, self.limit), min(hi, self.limit)
        return (self.limit - hi, self.limit - lo) if self.invert else (lo, hi)

    def _add_range(self, lo, hi):
        if hi > lo:
            self.inv.execute_masked_accumulate_range(self.coeffs.data_ptr(), self.work.data_ptr(), self.sum.data_ptr(), self.index.data_ptr(),
                                                     lo, hi, self.c, stream=self._st or 0)

    def start(self):
        """the rank's starting sum: DC everywhere (scan.c:377-383), the fill of scan indices [0, offset) (:389-417), and one range inverse
        over the loop's scan indices before f0 -- not contiguous with the fill when step > 1, hence two calls.  Rewinds to frame f0."""
        self._check(self.lib.dspfft_broadcast_dc(self.sum.data_ptr(), self.coeffs.data_ptr(), self.w * self.h, self.c, self._st))
        if self.fill:
            self._add_range(*self._mirror(0, self.offset))
        self._add_range(*self._mirror(self.offset * self.step, self.f0 * self.step))
        self.frame = self.f0

    def owner(self, i):
        """rank that emits loop frame i (None outside [offset, offset + nframes))"""
        if not self.offset <= i < self.offset + self.nframes:
            return None
        base, rem = divmod(self.nframes, self.G)          # shard_range: the first rem ranks hold base + 1 frames
        k = i - self.offset
        return k // (base + 1) if k < rem * (base + 1) else rem + (k - rem * (base + 1)) // base

    def next_frame(self):
        """adds frame self.frame (scan.c:421-459) and returns its number, or None when the rank's frames are done"""
        i = self.frame
        if i >= self.f1:
            return None
        if self.invert:
            self._add_range(*self._mirror(i * self.step, (i + 1) * self.step))
        else:
            self.inv.execute_masked_accumulate(self.coeffs.data_ptr(), self.work.data_ptr(), self.sum.data_ptr(), self.ids.data_ptr(), i, self.c,
                                               stream=self._st or 0)
        self.frame = i + 1
        return i


class FrameShardedZoom:
    """zoom's animation loop (zoom/zoom.c:320-410) with its frames spread over the ranks.  Frames are independent once the per-frame state
    (zoom.resolve_frames: the table of expression values applied in zoom.c:321-345's order) is resolved; every rank resolves the whole
    table (host-side and cheap), runs its own forward transform and renders the rendered frames shard_range deals it: no collective.
    With K frames kept on G ranks a rank renders at most ceil(K / G), so the ceiling of the speed-up is K / ceil(K / G) (4.0x for 240
    frames on 4 GPUs, 8.0x on 8; 3.5x for 7 frames on 4).  Frames come out on their owner only, as in FrameShardedScan.

    Every frame is chirp-z (dspfft_zoomanim_*); a geometry the chirp-z plans do not cover raises (Zoom.animation keeps the dense product)."""

    def __init__(self, image_hwc, vw, vh, table, present, basis_type=0, vx=0.0, vy=0.0, xscale=(1.0, 1.0), yscale=(1.0, 1.0),
                 showsamples=0, layout="rgb", group=None, lib=None, trc=0):
        import ctypes as C
        from . import _lib
        from .engine import trc_id
        from .zoom import resolve_frames, LAYOUTS
        self.lib = lib or _lib.load()
        self.G = dist.get_world_size(group) if dist.is_initialized() else 1
        self.rank = dist.get_rank(group) if dist.is_initialized() else 0
        self.h, self.w, c = image_hwc.shape
        assert c == 3 and image_hwc.dtype == torch.float32
        self.vw, self.vh, self.showsamples, self.layout = vw, vh, showsamples, LAYOUTS[layout]
        self.frames_all = list(resolve_frames(table, present, vx, vy, xscale, yscale))
        self.lo, self.hi = shard_range(len(self.frames_all), self.rank, self.G)
        self._st = SlabDCT3D._stream(image_hwc) or None
        self.coeffs = image_hwc.contiguous().clone()
        Plan.image(self.h, self.w, 3, REDFT10, lib=lib).execute(self.coeffs.data_ptr(), stream=self._st or 0)
        z = C.c_void_p()
        self._check(self.lib.dspfft_zoomanim_create(C.byref(z), self.w, self.h, basis_type, vw, vh))
        self.z = z
        self.work = torch.empty(self.lib.dspfft_zoomanim_work_floats(z), dtype=torch.float32, device=image_hwc.device)
        self._check(self.lib.dspfft_zoomanim_set_coeffs(z, self.coeffs.data_ptr(), self._st))
        self._check(self.lib.dspfft_zoomanim_set_trc(z, trc_id(trc, self.lib)))      # zoom -g: every output sample encoded

    def _check(self, rc):
        if rc:
            raise RuntimeError(self.lib.dspfft_zoomanim_last_error().decode())

    def owner(self, d):
        """rank that renders frame d (None for a skipped frame or one outside the table)"""
        for k, f in enumerate(self.frames_all):
            if f[0] == d:
                base, rem = divmod(len(self.frames_all), self.G)
                return k // (base + 1) if k < rem * (base + 1) else rem + (k - rem * (base + 1)) // base
        return None

    def frames(self):
        """yields (d, frame) for this rank's frames, in order: (vh, vw, 3), or (3, vh, vw) planes G, B, R"""
        shape = (self.vh, self.vw, 3) if self.layout == 0 else (3, self.vh, self.vw)
        for d, xs, ys, fx, fy in self.frames_all[self.lo:self.hi]:
            out = torch.empty(shape, dtype=torch.float32, device=self.coeffs.device)
            self._check(self.lib.dspfft_zoomanim_execute(self.z, float(xs[0]), float(xs[1]), float(ys[0]), float(ys[1]), float(fx), float(fy),
                                                         self.showsamples, self.layout, out.data_ptr(), self.work.data_ptr(), self._st))
            yield d, out

    def __del__(self):
        try:
            if getattr(self, "z", None) is not None:
                self.lib.dspfft_zoomanim_destroy(self.z)
                self.z = None
        except Exception:
            pass
