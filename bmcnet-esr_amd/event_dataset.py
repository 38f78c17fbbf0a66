"""Training from recordings kept on the GPU as raw event columns: the training counterpart of MultiStreamSR.open_events.

The reference trains from SequenceDataset (dataloader/h5dataset.py:637-700): per sequence L items of H5Dataset.__getitem__
(:261-316), each an HDF5 slice, flips and an index_put_ scatter in a loader worker.  Here the recordings stay on the GPU as the
dataset's raw columns (xs / ys int16, ps float64) and EventTrainSet.batch encodes every LR and HR frame of B sequences in ONE
launch (csrc/seq_encode.hip, bmc_seq_encode; include/bmc_hip.h "sequence encoder for training" states the contract) into the
collate layout train_step.bptt_step takes.  The host part is the reference's sequence sampling, bit for bit: the step size,
the seed and the flips one sequence shares, the pause chain, the noise events (sequence_plan, noise_events).

EventTrainSet(crop=(h, w), scale=s) trains on patches: every sample is an h x w LR patch and its s*h x s*w HR patch, cut at one
origin per sequence (crop_origin, drawn from the sequence's own seed; batch(origins=...) overrides it) out of the recording's own
frames, so recordings of different sensor sizes share a batch.  The crop happens in the encoder (bmc_seq_encode_crop): still one
table copy and one launch per batch, which writes only the patches -- bit for bit the slices of the full-frame batch.
With "Transpose" among the augmentation mechanisms (bit 3 of a sample's flags, this project's addition to the reference's three
flips) a sample's patch comes out of its transposed frames, in the same launch: all 8 orientations of a patch.

Out of scope, as in event_window_indices: HDF5 reading, the reference's 'time' / 'frame' modes, the hot-pixel filter (the
reference never applies it in training)."""
import random

import numpy as np
import torch

from bmc_hip import lib
from bmc_hip.encodings import check_hr_noise_filter, event_window_indices, filter_noise, synthesize_lr

MAX_ITEMS = lib.const("BMC_SEQ_MAX_ITEMS")
MAX_BATCH = 65535
MAX_WIDTH = 7680         # one row of both channels must fit a workgroup's LDS band
SEQ_SAMPLE_DTYPE = lib.dtype("bmc_seq_sample_t")
SEQ_CROP_DTYPE = lib.dtype("bmc_seq_crop_t")
ENCODE_LAUNCHES = 0      # bmc_seq_encode and bmc_seq_encode_crop launches of this process


def _augment_args(augment):
    """None (off) or (mechanisms, probs): config['data_augment']['augment'] / ['augment_prob'] of the reference."""
    if augment is None:
        return None
    try:
        mechanisms, probs = augment
        mechanisms, probs = tuple(mechanisms), tuple(float(p) for p in probs)
    except (TypeError, ValueError):
        raise ValueError("augment must be None or (mechanisms, probs)") from None
    if len(probs) < len(mechanisms):
        raise ValueError("augment: %d mechanisms, %d probabilities" % (len(mechanisms), len(probs)))
    return mechanisms, probs


def _pause_args(pause):
    """None (off) or (proba_pause_when_running, proba_pause_when_paused)."""
    if pause is None:
        return None
    try:
        running, paused = pause
        return float(running), float(paused)
    except (TypeError, ValueError):
        raise ValueError("pause must be None or (proba_pause_when_running, proba_pause_when_paused)") from None


TRANSPOSE = 8            # bit 3 of the flags: the sample's frames are transposed (patches only; bmc_seq_encode_crop)


def _flags_on(rng, seed, mechanisms, probs):
    """bmc_hip.encodings.augment_flags' rule on `rng`: augment_event (dataloader/h5dataset.py:559-578) re-seeds with seed,
    seed + 1, seed + 2 for Horizontal / Vertical / Polarity and draws once each; other names are skipped, as there.
    "Transpose" is this project's fourth mechanism in the same pattern: bit 3, rng.seed(seed + 3), one draw; a list that does
    not name it makes the calls it always made."""
    flags = 0
    for i, mech in enumerate(mechanisms):
        bit = {"Horizontal": 0, "Vertical": 1, "Polarity": 2, "Transpose": 3}.get(mech)
        if bit is None:
            continue
        rng.seed(seed + bit)
        if rng.random() < probs[i]:
            flags |= 1 << bit
    return flags


def sequence_plan(i, length, L, step_size=None, augment=None, pause=None, rng=random):
    """Sequence i of a recording of `length` items -> (seed, items, paused, flips): the L dataset items SequenceDataset.__getitem__
    (dataloader/h5dataset.py:666-700) reads, which of them it reads with Pause=True, the seed it hands to every item and the
    flip flags (bit0 horizontal, bit1 vertical, bit2 polarity) that seed gives.  Call for call on `rng` (the `random` module, or
    a random.Random): rng.randint(0, 2**32) for the seed; for every item, with augmentation on, the re-seeding draws of
    augment_event (the reference runs them twice per item, for the LR and the HR events: the second run leaves the same state
    and is not repeated here); between the items, with pause on, the chain's rng.random(), the item counter not advancing on a
    paused item (which is paired with the last item's ground truth).
    Kept, not fixed: with augmentation on every item re-seeds rng, so all pause draws of a sequence are the same number -- the
    second draw after rng.seed(seed + 2) when Polarity is the last mechanism, after rng.seed(seed + 3) when "Transpose" (bit3 of
    the flags; EventTrainSet with crop only) is.  Item 0 is never paused.
    step_size None: L, as the reference.  augment: None or (mechanisms, probs); pause: None or (proba_pause_when_running,
    proba_pause_when_paused).  L > length raises: the reference shortens that one sequence and its collate then fails."""
    L, length = int(L), int(length)
    step = L if step_size is None else int(step_size)
    if L < 1 or step < 1:
        raise ValueError("sequence_plan: L and step_size must be positive")
    if L > length:
        raise ValueError("sequence_plan: a sequence of L = %d items does not fit a recording of %d" % (L, length))
    n = (length - L) // step + 1
    if not 0 <= i < n:
        raise IndexError("sequence_plan: sequence %d of %d" % (i, n))
    augment, pause = _augment_args(augment), _pause_args(pause)
    seed = rng.randint(0, 2 ** 32)
    flips = 0
    j, k = int(i) * step, 0
    if augment is not None:
        flips = _flags_on(rng, seed, *augment)
    items, paused = [j], [False]
    now = False
    for _ in range(L - 1):
        if pause is not None:
            now = rng.random() < (pause[1] if now else pause[0])
        if not now:
            k += 1
        items.append(j + k)
        paused.append(now)
        if augment is not None:
            _flags_on(rng, seed, *augment)
    return seed, items, paused, flips


def noise_events(window, lr_size, seed, noise_level):
    """The noise events H5Dataset.add_noise_event (dataloader/h5dataset.py:623-634) appends to every LR item of a sequence with
    this seed -> (xs int16, ys int16, ps int8) numpy columns of int(window * noise_level) events: x = int(u0 * W), y = int(u1 * H),
    p = +-1 from u3, u = torch.rand([4, n]).  A local torch.Generator seeded with `seed` draws the same values as the reference's
    torch.manual_seed(seed) and leaves the global generator alone.  The float32 product can round up to W (or H): such an event
    is out of range and counts as one.  The columns are small integers and are made on the host."""
    H, W = (int(v) for v in lr_size)
    n = int(window * noise_level)
    g = torch.Generator()
    g.manual_seed(int(seed))
    u = torch.rand([4, n], generator=g)
    xs = (u[0] * W).int().to(torch.int16).numpy()
    ys = (u[1] * H).int().to(torch.int16).numpy()
    ps = ((u[3] * 2).int() * 2 - 1).to(torch.int8).numpy()
    return xs, ys, ps


def _max_origin(lr_size, gt_size, crop, scale):
    """The largest (top, left) at which the LR patch and its HR patch both lie inside their frames; negative: it does not fit."""
    (H, W), (gh, gw), (h, w) = lr_size, gt_size, crop
    return min(H - h, (gh - scale * h) // scale), min(W - w, (gw - scale * w) // scale)


def _oriented(size, transpose):
    """(H, W, gh, gw) as the sample's output sees them: swapped to (W, H, gw, gh) for a transposed sample."""
    H, W, gh, gw = size
    return (W, H, gw, gh) if transpose else (H, W, gh, gw)


def crop_origin(seed, lr_size, gt_size, crop, scale, transpose=False):
    """The patch origin (top, left), in LR image rows / columns, of a sequence with this seed (sequence_plan's): g =
    random.Random(seed); top = g.randint(0, max_top); left = g.randint(0, max_left), in that order, with max_top = min(H - h,
    (gh - scale * h) // scale) and max_left likewise -- the HR patch scale * (top, left) .. scale * (top + h, left + w) must fit
    a ground truth that may be smaller than scale x LR.  A generator of its own: the caller's rng is not touched, so cropping
    changes no plan.  transpose: the origin of a transposed sample (bit 3 of its flags), in the transposed frames' rows / columns:
    crop_origin on the swapped sizes (W, H), (gw, gh) -- the same draws in the same order."""
    lr_size, gt_size, crop = (tuple(int(v) for v in t) for t in (lr_size, gt_size, crop))
    if transpose:
        lr_size, gt_size = lr_size[::-1], gt_size[::-1]
    max_top, max_left = _max_origin(lr_size, gt_size, crop, int(scale))
    if max_top < 0 or max_left < 0:
        raise ValueError("crop_origin: a %dx%d patch (scale %d) does not fit frames %s -> %s" % (crop + (int(scale), lr_size, gt_size)))
    g = random.Random(seed)
    top = g.randint(0, max_top)
    return top, g.randint(0, max_left)


def _index_table(who, name, idx, n):
    a = np.asarray(idx.cpu() if torch.is_tensor(idx) else idx)
    if a.ndim != 2 or a.shape[1] != 2 or a.dtype.kind not in "iu":
        raise ValueError(who + "%s must be an integer [L,2] table (got %s %s)" % (name, a.dtype, a.shape))
    a = a.astype(np.int64)
    if (a[:, 0] > a[:, 1]).any():
        raise ValueError(who + "%s has a range with first > end" % name)
    if a.size and (a.min() < 0 or a.max() > n):
        raise ValueError(who + "%s has a range outside the %d events of its columns" % (name, n))
    return a


class EventTrainSet:
    """Recordings on the GPU as raw event columns -> training batches of count images, one launch per batch.

    L, step_size, augment, pause as sequence_plan; add_noise: None or the reference's noise_level; window: the LR events per
    item the noise count is taken from (config['window']).  Sequence indices run over the recordings in the order they were
    added, (length - L) // step_size + 1 each, as ConcatDataset over SequenceDataset.
    crop: None (full frames; all recordings share one pair of sizes) or (h, w): batches of h x w LR patches and scale*h x scale*w
    HR patches, from recordings of any sizes the patch fits.
    augment may name "Transpose" (a set with crop only: full frames of one size cannot hold a transposed sample): with the two
    flips, all 8 orientations of a patch.  The encoder cuts a transposed sample's patch out of its transposed frames, in the same
    launch as the others; the patch must fit every recording in both orientations."""
    RING = 2

    def __init__(self, L=9, step_size=None, augment=None, pause=None, add_noise=None, window=2048, crop=None, scale=4):
        self.L = int(L)
        if not 2 <= self.L <= MAX_ITEMS:
            raise ValueError("EventTrainSet: 2 <= L <= %d (got %d)" % (MAX_ITEMS, self.L))
        self.step_size = self.L if step_size is None else int(step_size)
        if self.step_size < 1:
            raise ValueError("EventTrainSet: step_size must be positive")
        self.augment, self.pause = _augment_args(augment), _pause_args(pause)
        self.noise_level = None if add_noise is None else float(add_noise)
        self.window = int(window)
        self.n_noise = 0 if self.noise_level is None else int(self.window * self.noise_level)
        self.crop, self.scale, self.last_origins, self.last_flips = None, int(scale), None, None
        self.transposes = self.augment is not None and "Transpose" in self.augment[0]
        if self.transposes and crop is None:
            raise ValueError('EventTrainSet: "Transpose" needs crop: full frames of one size cannot hold a transposed sample')
        if crop is not None:
            try:
                h, w = (int(v) for v in crop)
            except (TypeError, ValueError):
                raise ValueError("EventTrainSet: crop must be None or (h, w)") from None
            if min(h, w, self.scale) < 1 or self.scale * w > MAX_WIDTH:
                raise ValueError("EventTrainSet: crop and scale must be positive and scale * w at most %d (got crop %s, scale %d)"
                                 % (MAX_WIDTH, (h, w), self.scale))
            self.crop = (h, w)
        self._recs, self._ends, self._size, self._device = [], [], None, None
        self._pinned, self._events, self._table, self._k = None, [None] * self.RING, None, 0

    # ------------------------------------------------------------------ recordings
    def add_recording(self, lr, gt, lr_index, gt_index, lr_size, gt_size, noise_filter=None):
        """One recording -> its number.  lr, gt = (xs, ys, ps): 1-D int16, int16, float64 GPU tensors, polarities -1 / 0 / +1;
        lr_index, gt_index [length,2] integer tables on the host (bmc_hip.encodings.event_window_indices gives the reference's);
        every range is checked here against the column lengths: the kernel trusts the table.  All recordings share one pair
        of sizes; a set with crop takes any sizes the patch fits.
        noise_filter=dict(ts=, dt=, support=) (bmc_hip.encodings.check_noise_filter): the background-activity filter of
        include/bmc_hip_denoise.h runs once, here, over the whole LR stream, and the set holds the LR polarity column with the
        dropped events given weight +0.0 -- the recording trains as one added with (xs, ys, ps * keep); the caller's tensors
        are not modified, the ground truth is not filtered, noise_dropped() tells the count."""
        who = "EventTrainSet.add_recording: "
        for name, cols in (("lr", lr), ("gt", gt)):
            if not (isinstance(cols, (tuple, list)) and len(cols) == 3 and all(torch.is_tensor(t) for t in cols)):
                raise ValueError(who + "%s must be three tensors (xs, ys, ps)" % name)
            if [t.dtype for t in cols] != [torch.int16, torch.int16, torch.float64]:
                raise ValueError(who + "%s columns must be int16, int16, float64 (got %s)" % (name, [t.dtype for t in cols]))
            if any(t.dim() != 1 or t.numel() != cols[0].numel() or not t.is_contiguous() for t in cols):
                raise ValueError(who + "%s columns must be contiguous 1-D tensors of one length" % name)
        lr_index = _index_table(who, "lr_index", lr_index, lr[0].numel())
        gt_index = _index_table(who, "gt_index", gt_index, gt[0].numel())
        if len(lr_index) != len(gt_index):
            raise ValueError(who + "lr_index has %d rows, gt_index %d" % (len(lr_index), len(gt_index)))
        if len(lr_index) < self.L:
            raise ValueError(who + "%d items, fewer than one sequence of L = %d" % (len(lr_index), self.L))
        try:
            (H, W), (gh, gw) = (int(v) for v in lr_size), (int(v) for v in gt_size)
        except (TypeError, ValueError):
            raise ValueError(who + "lr_size = (H, W) and gt_size = (gh, gw)") from None
        if self.crop is not None:
            if min(H, W, gh, gw) < 1:
                raise ValueError(who + "sizes must be positive (got %s, %s)" % ((H, W), (gh, gw)))
            if min(_max_origin((H, W), (gh, gw), self.crop, self.scale)) < 0:
                raise ValueError(who + "the %dx%d patch (scale %d) does not fit the recording's %s -> %s"
                                 % (self.crop + (self.scale, (H, W), (gh, gw))))
            if self.transposes and min(_max_origin((W, H), (gw, gh), self.crop, self.scale)) < 0:
                raise ValueError(who + "the %dx%d patch (scale %d) does not fit the recording's %s -> %s transposed (%s -> %s)"
                                 % (self.crop + (self.scale, (H, W), (gh, gw), (W, H), (gw, gh))))
        elif min(H, W, gh, gw) < 1 or max(W, gw) > MAX_WIDTH:
            raise ValueError(who + "sizes must be positive and at most %d wide (got %s, %s)" % (MAX_WIDTH, (H, W), (gh, gw)))
        elif self._size is not None and self._size != (H, W, gh, gw):
            raise ValueError(who + "sizes differ: this set holds %s -> %s, the recording is %s -> %s"
                             % (self._size[:2], self._size[2:], (H, W), (gh, gw)))
        cols = tuple(lr) + tuple(gt)
        if not all(t.is_cuda and t.device == cols[0].device for t in cols) or (self._device or cols[0].device) != cols[0].device:
            raise ValueError(who + "the columns must be GPU tensors on one device")
        for name, ps in (("lr", lr[2]), ("gt", gt[2])):
            if not bool(((ps == 1) | (ps == -1) | (ps == 0)).all()):
                raise ValueError(who + "%s polarities must be -1, 0 or +1 (counts are integers)" % name)
        dropped = None
        if noise_filter is not None:
            lr, dropped = filter_noise(who, noise_filter, tuple(lr), (H, W))
            cols = tuple(lr) + tuple(gt)
        self._size, self._device = (H, W, gh, gw), cols[0].device
        self._recs.append(dict(cols=cols, ptrs=[t.data_ptr() for t in cols], lr_index=lr_index, gt_index=gt_index, size=(H, W, gh, gw),
                               noise_dropped=dropped))
        self._ends.append(len(self) + (len(lr_index) - self.L) // self.step_size + 1)
        return len(self._recs) - 1

    def add_hr_recording(self, gt, gt_ts, gt_size, window=2048, sliding_window=1024, threshold=None, dataset_length=None,
                         noise_filter=None):
        """One HR-ONLY recording -> its number.  gt = (xs, ys, ps) and gt_ts, the float64 timestamp column parallel to them
        (1-D GPU tensors), of a sensor of gt_size = (gh, gw).  The LR half is synthesized here, once, on the GPU, by integrate-and-
        fire over blocks of scale x scale pixels with the set's scale (bmc_hip.encodings.downsample_events, the contract:
        include/bmc_hip_downsample.h; threshold None = scale^2), both index tables are event_window_indices(lr_ts, gt_ts, window,
        sliding_window, scale, dataset_length) on the synthetic and the given timestamps, and the rest is add_recording: by
        construction the recording trains bit for bit as one added with the same LR columns made beforehand.
        noise_filter=dict(dt=, support=) needs no ts: the synthesized column is supplied, so the filter acts on the synthetic LR
        stream.  One host sync (the LR event count).  synthesized_events() tells the count; the caller's tensors are not
        modified."""
        who = "EventTrainSet.add_hr_recording: "
        noise_filter = check_hr_noise_filter(who, noise_filter)
        lr, lr_ts, lr_size = synthesize_lr(who, gt, gt_ts, gt_size, self.scale, threshold)
        try:
            lr_index, gt_index = event_window_indices(lr_ts.cpu().numpy(), gt_ts.cpu().numpy(), window, sliding_window, self.scale,
                                                      dataset_length)
        except ValueError as e:
            raise ValueError(who + "the %d synthesized LR events: %s" % (lr_ts.numel(), e)) from None
        if noise_filter is not None:
            noise_filter = dict(noise_filter, ts=lr_ts)
        r = self.add_recording(lr, gt, lr_index, gt_index, lr_size, gt_size, noise_filter=noise_filter)
        self._recs[r]["synthesized"] = lr_ts.numel()
        return r

    def synthesized_events(self, recording):
        """LR events synthesized for a recording added with add_hr_recording; None for one added with its own LR stream."""
        return self._recs[recording].get("synthesized")

    def noise_dropped(self, recording):
        """Events the noise filter dropped from the recording's LR stream; None for one added without noise_filter."""
        return self._recs[recording]["noise_dropped"]

    def __len__(self):
        return self._ends[-1] if self._ends else 0

    def locate(self, index):
        """Sequence index of the set -> (recording number, sequence number inside it)."""
        index = int(index)
        if not 0 <= index < len(self):
            raise IndexError("EventTrainSet: sequence %d of %d" % (index, len(self)))
        r = int(np.searchsorted(self._ends, index, side="right"))
        return r, index - (self._ends[r - 1] if r else 0)

    # ------------------------------------------------------------------ batches
    def plan(self, index, rng=random):
        """-> (recording number,) + sequence_plan(...) of sequence `index`."""
        r, i = self.locate(index)
        return (r,) + sequence_plan(i, len(self._recs[r]["lr_index"]), self.L, self.step_size, self.augment, self.pause, rng)

    def _orientation(self, transposed):
        """For messages: which frames of its recording a sample's plan drew; nothing where the set never transposes."""
        return "" if not self.transposes else ", transposed: its plan drew the transpose" if transposed else ", not transposed"

    def _buffers(self, B):
        """Pinned host copies (a ring: one is rewritten only after the copy that last read it has completed) and the device
        buffer of B table entries followed by B crop entries (a set with crop) and B noise column sets; grown when a larger
        batch comes."""
        nbytes = B * (SEQ_SAMPLE_DTYPE.itemsize + (SEQ_CROP_DTYPE.itemsize if self.crop else 0) + 8 * ((5 * self.n_noise + 7) // 8))
        if self._table is None or self._table.numel() < nbytes:
            torch.cuda.synchronize(self._device)
            self._pinned = [torch.zeros(nbytes, dtype=torch.uint8, pin_memory=True) for _ in range(self.RING)]
            self._events = [None] * self.RING
            self._table = torch.zeros(nbytes, dtype=torch.uint8, device=self._device)
        return nbytes

    def batch(self, indices, rng=random, origins=None):
        """Sequences `indices` of the set -> (inp_cnt [B,L,2,H,W], gt_cnt [B,L,2,gh,gw]) float32 on the GPU, the layout
        train_step.bptt_step takes: one table copy (entries and noise columns in one pinned buffer) and ONE bmc_seq_encode launch
        on the current stream.  The samples' plans draw from `rng` in the order of `indices`, as a loader worker would walk them.
        The pinned table and its device copy are reused between calls; the two results are new tensors.
        A set with crop = (h, w) returns the patches [B,L,2,h,w], [B,L,2,scale*h,scale*w] instead, from ONE bmc_seq_encode_crop
        launch (the crop entries travel in the same table copy, behind the sample entries): the slices of the full-frame batch
        at self.last_origins ([B,2] int64 numpy, (top, left) per sample), which are crop_origin of each plan's seed, or
        `origins` (integer [B,2]) where given.  The noise is drawn against each recording's own LR size.
        self.last_flips ([B] int64 numpy) holds each sample's flags.  A sample whose plan drew bit 3 ("Transpose") is the patch
        of its TRANSPOSED frames: full_inp[b].transpose(-1, -2)[..., top:top+h, left:left+w], its origin (crop_origin(...,
        transpose=True), or the one given) and its entry of last_origins in the transposed frames' rows / columns.  origins are
        checked after the plans are made, each against the orientation its sample drew; a refused batch leaves rng as it was."""
        global ENCODE_LAUNCHES
        from bmc_hip.encodings import encode_sequence_crops, encode_sequences
        who = "EventTrainSet.batch: "
        indices = [int(v) for v in indices]
        B = len(indices)
        if not 1 <= B <= MAX_BATCH:
            raise ValueError(who + "1 <= B <= %d sequences (got %d)" % (MAX_BATCH, B))
        if origins is not None:
            if self.crop is None:
                raise ValueError(who + "origins needs a set with crop")
            origins = np.asarray(origins.cpu() if torch.is_tensor(origins) else origins)
            if origins.shape != (B, 2) or origins.dtype.kind not in "iu":
                raise ValueError(who + "origins must be an integer [%d,2] array (got %s %s)" % (B, origins.dtype, origins.shape))
            origins = origins.astype(np.int64)
        state = None if origins is None else rng.getstate()
        plans = [self.plan(v, rng) for v in indices]
        if origins is not None:                                      # against the orientation each sample's plan drew
            for v, plan, (top, left) in zip(indices, plans, origins.tolist()):
                tr = bool(plan[4] & TRANSPOSE)
                size = _oriented(self._recs[plan[0]]["size"], tr)
                max_top, max_left = _max_origin(size[:2], size[2:], self.crop, self.scale)
                if not (0 <= top <= max_top and 0 <= left <= max_left):
                    rng.setstate(state)                              # a refused batch has drawn nothing
                    raise ValueError(who + "origin (%d, %d) of sequence %d lies outside (0, 0) .. (%d, %d), where the %dx%d patch "
                                     "fits its recording's %s -> %s%s" % ((top, left, v, max_top, max_left) + self.crop +
                                                                         (size[:2], size[2:], self._orientation(tr))))
        L, nn = self.L, self.n_noise
        nbytes = self._buffers(B)
        k = self._k
        if self._events[k] is not None:
            self._events[k].synchronize()
        host = self._pinned[k].numpy()
        tab = host[:B * SEQ_SAMPLE_DTYPE.itemsize].view(SEQ_SAMPLE_DTYPE)
        tab[:] = np.zeros((), SEQ_SAMPLE_DTYPE)
        crop_off = noise_off = B * SEQ_SAMPLE_DTYPE.itemsize
        if self.crop is not None:
            noise_off += B * SEQ_CROP_DTYPE.itemsize
            crops = host[crop_off:noise_off].view(SEQ_CROP_DTYPE)
            used = np.zeros((B, 2), np.int64)
        stride = 8 * ((5 * nn + 7) // 8)
        for b, (r, seed, items, paused, flips) in enumerate(plans):
            rec = self._recs[r]
            H, W, gh, gw = rec["size"]
            for name, p in zip(SEQ_SAMPLE_DTYPE.names[:6], rec["ptrs"]):
                tab[name][b] = p
            tab["lr_range"][b, :L] = rec["lr_index"][items]
            tab["gt_range"][b, :L] = rec["gt_index"][items]
            tab["flips"][b] = flips
            tab["paused"][b] = sum(1 << t for t, p in enumerate(paused) if p)
            if self.crop is not None:
                used[b] = origins[b] if origins is not None else crop_origin(seed, (H, W), (gh, gw), self.crop, self.scale,
                                                                             bool(flips & TRANSPOSE))
                crops[b] = (H, W, gh, gw, used[b, 0], used[b, 1])    # the recording's own sizes, never swapped
            if nn:
                off = noise_off + b * stride
                xs, ys, ps = noise_events(self.window, (H, W), seed, self.noise_level)
                host[off:off + 2 * nn].view(np.int16)[:] = xs
                host[off + 2 * nn:off + 4 * nn].view(np.int16)[:] = ys
                host[off + 4 * nn:off + 5 * nn].view(np.int8)[:] = ps
                base = self._table.data_ptr() + off
                tab["noise_xs"][b], tab["noise_ys"][b], tab["noise_ps"][b], tab["n_noise"][b] = base, base + 2 * nn, base + 4 * nn, nn
        with torch.cuda.device(self._device):
            self._table[:nbytes].copy_(self._pinned[k][:nbytes], non_blocking=True)
            ev = self._events[k] = self._events[k] or torch.cuda.Event()
            ev.record()
            self._k = (k + 1) % self.RING
            if self.crop is None:
                out = encode_sequences(self._table, B, L, self._size[:2], self._size[2:])
            else:
                out = encode_sequence_crops(self._table, self._table[crop_off:noise_off], B, L, self.crop, self.scale)
                self.last_origins = used
        self.last_flips = np.asarray([p[4] for p in plans], np.int64)
        ENCODE_LAUNCHES += 1
        return out

    def batches(self, batch_size, shuffle=True, drop_last=True, generator=None, rank=0, world=1):
        """Index lists for one epoch -> list of lists for batch().  The order is torch.randperm(len, generator=generator) when
        shuffle (else 0 .. len-1), padded by its own head to a multiple of `world`; rank r takes every world-th index from r --
        DistributedSampler's rule (the reference's loader, dataloader/h5dataloader.py:191-201) -- and cuts its share into
        batches of batch_size, the last short one dropped with drop_last."""
        n, world, rank, batch_size = len(self), int(world), int(rank), int(batch_size)
        if batch_size < 1 or world < 1 or not 0 <= rank < world:
            raise ValueError("EventTrainSet.batches: batch_size >= 1 and 0 <= rank < world")
        order = torch.randperm(n, generator=generator).tolist() if shuffle else list(range(n))
        total = -(-n // world) * world
        while n and len(order) < total:
            order += order[:total - len(order)]
        mine = order[rank:total:world]
        out = [mine[a:a + batch_size] for a in range(0, len(mine), batch_size)]
        if drop_last and out and len(out[-1]) < batch_size:
            out.pop()
        return out
