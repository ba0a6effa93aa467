"""A scene's source frames kept in memory in their stored form, and the loaders' items built from them (``resident=True``).

An item of the five loaders (the four of the NVIDIA family and the DyCheck iPhone one) stacks 20-odd source views, each
decoded from an image, a mask and a depth file, and a scene has only as many distinct source frames as its monocular video
(DyCheck: its train camera): frame ``i`` is always the same files.  ``SceneStore`` decodes a frame on its first use, through
the loader's own readers, and keeps per scene

  rgb       uint8   [F,H,W,3]  the pixels before ``/ 255``
  dyn_mask  uint8   [F,H,W]    the mask file's values (0 / 1 for the 1-bit files)
  depth     float32 [F,H,W]    after the loader's resize, cast as ``F32`` casts it

each frame in a slot padded to a multiple of 16 bytes, a host bitmap of the filled slots, and the flow pairs ``(a, b)`` read so
far: ``flow`` float32 [H,W,2] and the occlusion mask [H,W] computed once, when the file is read.  With ``device=None`` the
tables are host memory and an item's views are gathered with numpy, statement for statement the disk path's; with a GPU
``device`` they live there and ``ops.item_views`` writes all of an item's views in one launch (``ops.flow_occ`` the occlusion
mask), bit-identical.  Once its frames are in, building an item on the GPU never waits for the device.

Slots are addressed by frame id: frame ``f`` of a scene lives in slot ``f - first_id``.  The NVIDIA-family loaders' frame
ids are the monocular video's indices (``first_id`` 0); the DyCheck loader's are its train camera's time ids, a consecutive
run that need not start at 0 (``first_id`` = the smallest; the scene has as many slots as train frames).  An id outside the
run is refused before anything is decoded.

A scene may be opened in "prediction" mode (the NVIDIA evaluation loader's ZoeDepth inputs): the ``depth`` table then holds
each frame's monocular prediction ``depth_pred`` as float32 and the scene keeps, on the host, the float64 (scale, shift) its
file stores for the pair the loader selected, both written when the slot is filled.  The aligned depth is not stored: under
NumPy 2 it is float64, the item carries its float32 rounding and ``depth_range`` is taken over the float64 cloud, so the
alignment (three pointwise lines) is restated per item, by ``zoe_align`` on a host store and by ``ops.item_zoe_depth`` on a
GPU store, which writes the float32 depths of all groups and selects the range over the float64 ones in one launch.

``resident_scenes`` most recently used scenes stay; ``resident_max_bytes`` caps the store: a scene whose tables alone exceed
it is refused before anything is allocated, older scenes and then the least recently used flow pairs go when it is reached.

A frame's input has six options, each building on another.  ``_common.device_input`` is the one statement of the first five
rules and ``_common.device_depth`` of the sixth, for the five loaders and for this store alike; the first rule broken, in this
order, is refused with what is missing:

  device_entropy  needs device_decode
  device_png      needs device_resize (it is independent of device_decode)
  device_mask     needs device_resize (it is independent of the others)
  device_decode   needs device_resize
  device_resize   needs resident=True, and the store on a GPU
  device_depth    needs device_resize (checked behind the five; it is independent of the others)

``device_resize``: the loaders hand over a frame's image as decoded, at the file's size, and the store uploads the bytes and
resizes them on the device straight into the frame's slot (``ops.resample_u8``, Pillow's BOX filter bit for bit); the
evaluation loaders' target image goes the same way (``expand_target``) and the pure-geometry loader's LANCZOS stack in one
batched call (``resize_stack``).  An image the device path does not serve (not uint8 [H,W,3], or a size ``ops.resample_plan``
refuses) takes the host statements.  Depths keep their host NEAREST resize unless ``device_depth`` is on, masks unless
``device_mask`` is.

``device_mask`` (``decode_mask``): a frame's mask file -- a non-interlaced grey or palette PNG of bit depth 1, 2, 4
or 8 (``ops.png_decode_batch(kinds="mask")``) -- is inflated, unfiltered and unpacked in HIP straight into ``dyn_mask[slot]``, or,
where the file has another size, gathered there through Pillow's own NEAREST picks (``ops.mask_place``); byte for byte the host
statement ``resize(np.array(PIL.Image.open(f)), h, w, NEAREST)``, which still takes every other file (16-bit, grey + alpha,
interlaced, tRNS, damaged, not a PNG ...), errors included.  The loaders name the files (``mask_path``) and ``_fill`` puts the
missing frames' masks into the same batch as their images when ``device_png`` is on as well -- one launch pair and one wait per
item fill -- or into one batch of their own.  The DyCheck covisible PNG goes the same way (``decode_mask`` at the file's size,
then ``ops.item_target``), the NVIDIA evaluation mask through ``decode_eval_mask``.  ``stats["masks_decoded_on_device"]`` and
``stats["mask_fallbacks"]`` count the outcomes; they exist under the option alone.

``device_depth`` (``_stage_depths``): a frame's depth file -- an ``.npy``, or a stored member of an ``.npz``, holding
little-endian float32 in C order (``npy_file`` finds the payload; no array is made on the host) -- crosses the bus as stored.  The
loaders name the file and their statement over it (``depth_request``: "reciprocal" ``1 / (disp + 1e-8)`` for the NVIDIA family,
"copy" for ``mono_vis`` and the ZoeDepth predictions, "scale" ``depth * scale`` for DyCheck); ``_fill`` gathers the missing frames'
payloads in one pinned buffer, uploads it once, and ONE ``ops.depth_place`` writes the float32 depths straight into
``depth[slot]``, through Pillow's own NEAREST picks where a file has another size: bit for bit the host statements, which still
take every other file (float16, float64, big-endian, Fortran order, a compressed member, damaged ...), errors included.
``stats["depths_placed_on_device"]`` and ``stats["depth_fallbacks"]`` count the outcomes; they exist under the option alone.  With
``device_png`` and ``device_mask`` on as well, an item fill touches no pixel on the host.  Under the option a GPU store also reads
a flow pair once, as stored, in one copy (``_upload_flow_pair``), and ``mono_vis`` takes its near depths from
``ops.percentile_f32`` over the uploaded payloads (``depth_percentiles``).

Three of the others decode images on the device, and ``decode_image`` is their one dispatch: it takes the file's bytes (from
``prefetch_images``' table, else from the file), asks the codec their signature names, counts the outcome, and hands every file
no codec serves to Pillow as before, errors included.  An image decoded there is byte for byte ``np.array(PIL.Image.open(path))``;
the store takes it where it takes a host one -- no second upload -- and a frame of the slot's size is decoded straight into its
slot (``_slot_for``).
``device_decode`` (``_decode_jpeg``): a JPEG stream that ``ops.jpeg_decode`` serves (baseline YCbCr, 4:4:4 / 4:2:2 /
4:2:0), Huffman scan on the host, everything behind it in HIP; not served (``stats["jpeg_fallbacks"]``): progressive, greyscale,
CMYK, truncated ... streams.  ``device_entropy`` (7i): the scan on the device as well: the file's bytes cross the bus, not its
coefficients, and ``decode_image`` waits once per file for the scan's status word; a scan the device gives up
(``stats["entropy_fallbacks"]``) is read again by the host decoder.
``device_png`` (``_decode_png``; 7j): non-interlaced 8-bit RGB and RGBA files are inflated and unfiltered in HIP
(``ops.png_decode_batch``; ``channels="rgb"``: the first three channels); not served (``stats["png_fallbacks"]``): another colour type
or bit depth, interlace, tRNS, a damaged file ...  ``prefetch_images`` decodes several files in one batched launch and one wait
and keeps the results for the ``decode_image`` calls that follow; ``views`` prefetches an item's missing frames that way where
the loader names their files (``image_path``).
"""
from collections import OrderedDict, namedtuple

import numpy as np
import PIL.Image
import torch

from . import _common
from ._common import F32, read_flow_npz, resize

DEFAULT_MAX_BYTES = 4 << 30
VIEW_KEYS = ("rgb", "dyn_rgb", "static_rgb", "dyn_mask", "depth")


def _pad16(nbytes):
    return -(-nbytes // 16) * 16


def table_bytes(n_frames, h, w):
    """bytes of one scene's three frame tables, the slots padded"""
    n = h * w
    return n_frames * (_pad16(n * 3) + _pad16(n) + _pad16(n * 4))


class _Scene:
    def __init__(self, n_frames, h, w, device, first_id=0, prediction=False):
        n = h * w
        self.n_frames, self.h, self.w, self.first_id = n_frames, h, w, int(first_id)
        self.prediction = bool(prediction)  # the depth table holds depth_pred; scale_shift[slot] aligns it
        self.scale_shift = np.zeros((n_frames, 2), np.float64) if prediction else None  # host, as the files give them
        self.zoe_pairs = [None] * n_frames if prediction else None  # (model type, principle) the slot was filled from
        self.filled = np.zeros(n_frames, dtype=bool)  # host bitmap of the decoded slots
        tab = lambda slot, dtype: torch.empty((n_frames, slot), dtype=dtype, device=device)  # noqa: E731
        self.rgb = tab(_pad16(n * 3), torch.uint8)[:, :n * 3].view(n_frames, h, w, 3)
        self.dyn_mask = tab(_pad16(n), torch.uint8)[:, :n].view(n_frames, h, w)
        self.depth = tab(_pad16(n * 4) // 4, torch.float32)[:, :n].view(n_frames, h, w)
        self.nbytes = table_bytes(n_frames, h, w)
        self.flows = OrderedDict()  # (a, b) -> (flow [H,W,2], occ [H,W]), least recently used first


# a file ``prefetch_images`` read, until the one ``decode_image`` that takes it: its bytes, what the PNG path decoded (None: refused,
# given up, or not a PNG) and whether that path has had its turn
_Prefetched = namedtuple("_Prefetched", "data image png_tried", defaults=(None, False))
# one file of a ``_png_decode`` batch: its bytes; "file" or "rgb" (an image, read with these ``channels``) or "mask"; a mask's wanted
# shape (None: the file's size); ``into`` = (scene or None, frame id), as ``decode_image`` and ``decode_mask`` take it
_PngRequest = namedtuple("_PngRequest", "data kind shape into")
# a frame's depth as ``_fill`` staged it under ``device_depth`` (``SceneStore.staged_depth``)
_StagedDepth = namedtuple("_StagedDepth", "depth data")


class SceneStore:
    """The per-dataset store.  ``device``: None (host memory, numpy gather) or a GPU device (``ops.item_views``).  The five
    image-input ``device_*`` keywords (the module's text), or ``device_input``: the loader's checked record of them; and
    ``device_depth``, the sixth, its own keyword either way."""

    def __init__(self, device=None, resident_scenes=1, resident_max_bytes=DEFAULT_MAX_BYTES, occ_thres=1.0, device_resize=False,
                 device_decode=False, device_entropy=False, device_png=False, device_input=None, device_mask=False, device_depth=False):
        if resident_scenes < 1 or resident_max_bytes < 0:
            raise ValueError(f"resident_scenes {resident_scenes} (>= 1), resident_max_bytes {resident_max_bytes} (>= 0)")
        self.device = None if device is None else torch.device(device)
        if self.device is not None and self.device.type != "cuda":
            raise ValueError(f"SceneStore: device None (host memory) or a GPU, got {self.device}")
        if type(occ_thres) not in (int, float):  # (np.float64 is a float subclass)
            raise TypeError(f"flow_consist_thres must be a Python number (a NumPy scalar changes the compare's type), got {type(occ_thres)}")
        self.resident_scenes, self.resident_max_bytes, self.occ_thres = int(resident_scenes), int(resident_max_bytes), occ_thres
        self.scenes = OrderedDict()  # key -> _Scene, least recently used first
        if device_input is None:  # the five keywords themselves: the loaders' one check, in the store's name
            device_input = _common.device_input("SceneStore", resident=True, device=self.device, device_resize=device_resize, device_decode=device_decode,
                                                device_entropy=device_entropy, device_png=device_png, device_mask=device_mask)
        self.device_resize, self.device_decode, self.device_entropy, self.device_png, self.device_mask = device_input
        self.device_depth = _common.device_depth("SceneStore", device_input, device_depth)  # (the sixth keyword: checked behind the five)
        self._staged_depths = {}  # (id(scene), frame id) -> _StagedDepth, from _fill's one depth_place until the frame's decode takes it
        self._prefetched = {}  # (path, channels or "mask") -> _Prefetched, from prefetch_images until decode_image / decode_mask hands it out
        self.stats = {"frames_decoded": 0, "flow_files_read": 0, "items_built": 0, "frames_resized_on_device": 0,
                      "targets_resized_on_device": 0, "zoe_files_read": 0, "frames_decoded_on_device": 0, "targets_decoded_on_device": 0,
                      "jpeg_fallbacks": 0, "scans_decoded_on_device": 0, "entropy_fallbacks": 0, "png_decoded_on_device": 0, "png_fallbacks": 0}
        if self.device_mask:  # (counted under the option alone: without it the record is the one it was)
            self.stats.update(masks_decoded_on_device=0, mask_fallbacks=0)
        if self.device_depth:
            self.stats.update(depths_placed_on_device=0, depth_fallbacks=0)

    @property
    def nbytes(self):
        return sum(s.nbytes + sum(self._pair_bytes(s, pair) for pair in s.flows.values()) for s in self.scenes.values())

    @staticmethod
    def _pair_bytes(scene, pair=None):
        """a flow pair's bytes: flow and occlusion mask; a pair read under ``device_depth`` keeps the uploaded buffer its flow is a
        view of, coord_diff included"""
        held = 0 if pair is None else max(pair[0].untyped_storage().nbytes() - scene.h * scene.w * 8, 0)
        return scene.h * scene.w * 12 + held

    # ------------------------------------------------------------------ scenes
    def scene(self, key, n_frames, shape, first_id=0, prediction=False):
        """the scene's tables, made on first use (nothing is decoded yet); the least recently used scenes leave.  Frame id
        ``f`` lives in slot ``f - first_id``.  ``prediction``: the depth table holds ZoeDepth predictions (the module's text)"""
        s = self.scenes.get(key)
        if s is not None:
            assert (s.n_frames, s.h, s.w, s.first_id, s.prediction) == (n_frames, *shape, first_id, bool(prediction)), (
                key, (s.n_frames, s.h, s.w, s.first_id, s.prediction), n_frames, shape, first_id, prediction)
            self.scenes.move_to_end(key)
            return s
        need = table_bytes(n_frames, *shape)
        if need > self.resident_max_bytes:
            raise ValueError(f"scene {key!r}: the tables of {n_frames} frames of {shape[0]} x {shape[1]} take {need} bytes, "
                             f"resident_max_bytes is {self.resident_max_bytes}")
        while len(self.scenes) >= self.resident_scenes:
            self.scenes.popitem(last=False)
        while self.scenes and self.nbytes + need > self.resident_max_bytes:  # flow pairs go first, then the oldest scene
            if not self._drop_flow_pair():
                self.scenes.popitem(last=False)
        s = self.scenes[key] = _Scene(n_frames, shape[0], shape[1], self.device, first_id, prediction)
        return s

    def _drop_flow_pair(self, keep=None):
        """drop the least recently used flow pair of the least recently used scene that has one; False when there is none"""
        for s in self.scenes.values():
            for k in s.flows:
                if (s, k) != keep:
                    del s.flows[k]
                    return True
        return False

    # ------------------------------------------------------------------ frames
    @staticmethod
    def slots(scene, frame_ids):
        """the frame ids' slots; an id outside the scene's run is refused (an index below 0 would wrap around)"""
        slots = [int(f) - scene.first_id for f in frame_ids]
        if slots and not 0 <= min(slots) <= max(slots) < scene.n_frames:
            raise ValueError(f"frame ids {[int(f) for f in frame_ids]} outside the scene's {scene.first_id}..{scene.first_id + scene.n_frames - 1}")
        return slots

    def _fill(self, scene, frame_ids, decode, image_path=None, mask_path=None, *, depth_request=None):
        missing = [f for f in sorted(set(frame_ids)) if not scene.filled[f - scene.first_id]]
        images = self.device_png and image_path is not None
        masks = [(mask_path(f), (scene.h, scene.w), (scene, f)) for f in missing] if self.device_mask and mask_path is not None else []
        if masks or (images and len(missing) > 1):  # the item's missing frames, images and masks, in one launch, one wait
            paths = [image_path(f) for f in missing] if images else []
            self.prefetch_images([p if isinstance(p, tuple) else (p, "file") for p in paths], [(scene, f) for f in missing], masks=masks)
        try:
            if self.device_depth and depth_request is not None and missing:  # the missing frames' depth payloads: one buffer, one copy, one launch
                self._stage_depths(scene, missing, depth_request)
            for f in missing:
                self.put(scene, f, *decode(f))
        finally:
            self._prefetched.clear()  # (also when a reader raises: the entries hold device tensors, some of them slots)
            self._staged_depths.clear()

    # ------------------------------------------------------------------ the depth files on the device
    def _stage_depths(self, scene, frames, depth_request):
        """``device_depth``: ``depth_request(frame id) -> (path or bytes, member or None, op, scale)`` names each
        frame's depth file -- an ``.npy``, or the stored member of an ``.npz`` -- and the statement the loader makes of it
        (``ops.DEPTH_OPS``; None: the loader has no float32 statement for this frame).  The payloads ``npy_file`` finds (float32,
        C order, [h,w]; with "scale", the DyCheck files' [h,w,1] too) cross the bus as stored in ONE pinned buffer and ONE
        ``ops.depth_place`` writes them straight into ``scene.depth[slot]``, through Pillow's NEAREST picks where a file has
        another size.  ``staged_depth`` hands each frame's outcome to its decode; a file the reader refuses is left to the loader's
        own host statement, errors included."""
        from .. import ops
        from . import npy_file

        placed, staged = [], {}
        for f, slot in zip(frames, self.slots(scene, frames)):
            request, data, served = depth_request(f), None, None
            if request is not None:
                source, member, op, scale = request
                raw = data = source if isinstance(source, (bytes, bytearray, memoryview)) else None
                if raw is None:
                    try:
                        with open(source, "rb") as fh:
                            raw = fh.read()
                    except OSError:  # (a missing file: the host statement says so)
                        raw = None
                if raw is not None:
                    offset, shape, _ = npy_file.npy_payload(raw) if member is None else npy_file.npz_member(raw, member)
                    if offset is not None and op == "scale" and len(shape) == 3 and shape[2] == 1:
                        shape = shape[:2]
                    if offset is not None and len(shape) == 2 and 1 <= min(shape) and max(shape) <= 16384:
                        served = ops.DepthRequest(raw, offset, shape, op, scale, scene.depth[slot])
            if served is not None:
                placed.append(served)
            staged[id(scene), int(f)] = _StagedDepth(None if served is None else served.out, data)
        if placed:
            ops.depth_place(placed, device=self.device)
        self._staged_depths.update(staged)
        self.stats["depths_placed_on_device"] += len(placed)
        self.stats["depth_fallbacks"] += len(frames) - len(placed)

    def staged_depth(self, scene, f):
        """what ``_fill`` staged for frame id ``f`` of ``scene`` under ``device_depth``: a ``_StagedDepth`` -- ``depth``: the frame's
        slot, filled on the device (``put`` recognises it), or None: the loader's host statement reads the file; ``data``: the
        file's bytes where the loader's request handed bytes over -- or None outside such a fill"""
        return self._staged_depths.get((id(scene), int(f))) if scene is not None else None

    def depth_percentiles(self, files, member, q):
        """``np.percentile(np.load(file)[member].reshape(-1), q)`` of every ``.npz`` file as a list of NumPy scalars (``mono_vis``'
        near depths).  Under ``device_depth`` each file is read once, the payloads of the members ``npy_file`` serves travel in
        ONE pinned buffer, ``ops.percentile_f32`` selects on the device and the host waits once; a file the reader refuses takes
        the host statement from the same bytes."""
        import io

        from .. import ops
        from . import npy_file

        out, spans, total = [None] * len(files), [], 0
        for i, path in enumerate(files):
            with open(path, "rb") as fh:
                data = fh.read()
            offset, shape, _ = npy_file.npz_member(data, member) if self.device_depth else (None, None, None)
            count = 0 if offset is None else int(np.prod(shape, dtype=np.int64))
            if 1 <= count < 1 << 31:
                spans.append((i, data, offset, total, count))
                total += _pad16(count * 4)
            else:
                out[i] = np.percentile(np.load(io.BytesIO(data))[member].reshape(-1), q)
        if spans:
            host = torch.empty(total, dtype=torch.uint8, pin_memory=True)
            view = host.numpy()
            for _, data, offset, at, count in spans:
                view[at:at + count * 4] = np.frombuffer(data, np.uint8, count * 4, offset)
            dev = host.to(self.device, non_blocking=True)
            got = ops.percentile_f32([dev[at:at + count * 4].view(torch.float32) for *_, at, count in spans], q).cpu().numpy()  # the one wait
            for (i, *_), value in zip(spans, got):
                out[i] = value
        return out

    # ------------------------------------------------------------------ the decode on the device
    def _slot_for(self, into, height, width, channels=3):
        """the slot ``into`` = (scene or None, frame id) names, where an image of this size is exactly what it keeps"""
        if into is None or into[0] is None or (height, width, channels) != (into[0].h, into[0].w, 3):
            return None
        return into[0].rgb[self.slots(into[0], [into[1]])[0]]

    def _png_decode(self, requests):
        """The PNG files of ``requests`` (``_PngRequest``) on the device, position for position: an image, a mask at its ``shape``
        (in its slot where ``into`` names one), or None where the host side refuses the file or the device gives it up.  Each
        file is walked once and its slot picked; then ONE batched launch with one wait per channels mode among the images.  The
        masks (``device_mask``) ride with the first mode's batch, or make one of their own where there is no image."""
        from .. import ops

        results, walked = [None] * len(requests), {}  # walked: position -> (what png_parse gave, the decode's out, a mask's slot)
        for i, r in enumerate(requests):
            mask = r.kind == "mask"
            if mask and ops.image_kind(r.data) != "png":
                continue
            parsed = ops.png_parse(r.data, kinds=("mask",) if mask else ("colour",))  # (the one chunk walk of this file)
            info = parsed[0]
            if info is None:
                continue
            if not mask:
                slot = self._slot_for(r.into, info["height"], info["width"], 3 if r.kind == "rgb" else info["channels"])
                walked[i] = (parsed, slot, slot)
            else:
                fits = r.shape is not None and r.into is not None and r.into[0] is not None and tuple(r.shape) == (r.into[0].h, r.into[0].w)
                slot = r.into[0].dyn_mask[self.slots(r.into[0], [r.into[1]])[0]] if fits else None
                same = r.shape is None or (info["height"], info["width"]) == tuple(r.shape)
                walked[i] = (parsed, slot if same else None, slot)
        masks = [i for i in walked if requests[i].kind == "mask"]
        for channels in list(dict.fromkeys(r.kind for r in requests if r.kind != "mask")) or ["file"]:
            batch = [i for i in walked if requests[i].kind == channels] + masks
            if not batch:
                continue
            got = ops.png_decode_batch([requests[i].data for i in batch], outs=[walked[i][1] for i in batch], channels=channels, device=self.device,
                                       reject_ok=True, parsed=[walked[i][0] for i in batch], kinds=("colour", "mask") if masks else ("colour",))
            for i, image in zip(batch, got):
                shape = requests[i].shape
                if image is not None and shape is not None and tuple(image.shape) != tuple(shape):
                    image = ops.mask_place(image, shape, out=walked[i][2])  # a mask of another size: Pillow's NEAREST picks, gathered on the device
                results[i] = image
            masks = []
        return results

    def prefetch_images(self, paths, intos=None, masks=()):
        """With ``device_png``: the files of ``paths`` (each a path, or (path, channels)) read once, and the PNG files among
        them decoded in ONE batched launch with one wait.  Bytes and outcome are kept for the ``decode_image`` calls that
        follow, which then neither read, parse nor launch again (``_fill`` and ``decode_stack`` drop what is left).  ``intos``:
        per path None or (scene, frame id), as ``decode_image`` takes it.  With ``device_mask``: ``masks`` = [(path, shape,
        into)], the mask files ``decode_mask`` will be asked for, in the same launch and wait as the images (or, without
        ``device_png``, in one of their own)."""
        masks = list(masks) if self.device_mask else []
        if not self.device_png and not masks:
            return
        from .. import ops

        paths = [p if isinstance(p, tuple) else (p, "file") for p in paths] if self.device_png else []
        intos = [None] * len(paths) if intos is None else intos
        wanted = [(path, channels, None, into) for (path, channels), into in zip(paths, intos)]
        wanted += [(path, "mask", shape, into) for path, shape, into in masks]
        keys, requests = [], []
        for path, kind, shape, into in wanted:
            key = (str(path), kind)
            if key in self._prefetched:
                continue
            with open(path, "rb") as f:
                data = f.read()
            is_png = kind == "mask" or ops.image_kind(data) == "png"  # (a mask file goes to the one batch function whatever it holds)
            self._prefetched[key] = _Prefetched(data, None, is_png)
            if is_png:
                keys.append(key)
                requests.append(_PngRequest(data, kind, shape, into))
        for key, request, image in zip(keys, requests, self._png_decode(requests)):
            self._prefetched[key] = _Prefetched(request.data, image, True)

    def decode_stack(self, paths):
        """``decode_image`` of every file as host arrays (the pure-geometry loader's stack, which ``resize_stack`` and the
        cloud take from the host): the PNG files among them decoded in one batched launch, then copied back"""
        self.prefetch_images(list(paths))
        try:
            images = [self.decode_image(p) for p in paths]
        finally:
            self._prefetched.clear()
        return [im.cpu().numpy() if isinstance(im, torch.Tensor) else im for im in images]

    def decode_image(self, path, target=False, into=None, channels="file"):
        """An image file's pixels: ``np.array(PIL.Image.open(path))``, or -- a PNG file under ``device_png``, a JPEG stream under
        ``device_decode``, by the file's bytes, not its name, where its codec below serves it -- the same bytes as a uint8 [H,W,C]
        tensor on the store's device (a JPEG without a wait unless ``device_entropy``, a PNG after one).  ``target``: counted as
        an item's target, not as a source frame.  ``into`` = (scene or None, frame id): a frame of the slot's size is decoded
        straight into ``scene.rgb[slot]``, which ``put`` then recognises.  ``channels="rgb"``: the first three channels of an RGBA
        image (``[..., :3]`` of Pillow's array; the DyCheck reader's)."""
        if self.device_decode or self.device_png:
            from .. import ops

            got = self._prefetched.pop((str(path), channels), None)
            if got is None:
                with open(path, "rb") as f:
                    got = _Prefetched(f.read())
            kind, image = ops.image_kind(got.data), None
            if kind == "png" and self.device_png:
                image = self._decode_png(got, into, channels)
            elif kind == "jpeg" and self.device_decode:
                image = self._decode_jpeg(got.data, into)
            if image is not None:
                self.stats["targets_decoded_on_device" if target else "frames_decoded_on_device"] += 1
                return image
        image = np.array(PIL.Image.open(path))
        return image[..., :3] if channels == "rgb" else image

    def decode_mask(self, path, shape=None, into=None):
        """A mask file's values at ``shape`` (None: the file's size): ``resize(np.array(PIL.Image.open(path)), *shape, NEAREST)``
        -- the loaders' host statement, which also takes every file the device path does not serve, errors included -- or,
        under ``device_mask`` and for a non-interlaced grey or palette PNG of bit depth 1, 2, 4 or 8, the same values as a uint8
        [h,w] tensor on the store's device (bool becomes 0 / 1, as the table keeps it): decoded by
        ``ops.png_decode_batch(kinds="mask")`` and, where the file has another size, gathered through Pillow's own NEAREST
        picks (``ops.mask_place``).  ``into`` = (scene or None, frame id): the mask lands in ``scene.dyn_mask[slot]`` itself,
        which ``put`` then recognises.  One wait, unless ``prefetch_images`` has had the file in its batch."""
        if self.device_mask:
            got = self._prefetched.pop((str(path), "mask"), None)
            if got is None:
                with open(path, "rb") as f:
                    got = _Prefetched(f.read())
            mask = got.image if got.png_tried else self._png_decode([_PngRequest(got.data, "mask", shape, into)])[0]
            self.stats["mask_fallbacks" if mask is None else "masks_decoded_on_device"] += 1
            if mask is not None:
                return mask
        mask = np.array(PIL.Image.open(path))
        return mask if shape is None else resize(mask, *shape, PIL.Image.Resampling.NEAREST)

    def decode_eval_mask(self, path, shape):
        """the NVIDIA evaluation mask ``np.float32(np.array(PIL.Image.open(path).convert("RGB"))[..., ::-1] > 1e-3)`` as a float32
        [h,w,3] tensor on the store's device, where ``device_mask`` serves it: a grey PNG (through the mask path) or an 8-bit RGB
        one (through the colour path) of exactly ``shape``, expanded by ``ops.mask_place``; else None -- a palette file, another
        size, anything the decode refuses or gives up -- and the caller's host statement reads the file.  One wait."""
        from .. import ops

        with open(path, "rb") as f:
            data = f.read()
        parsed = ops.png_parse(data, kinds=("colour", "mask")) if ops.image_kind(data) == "png" else (None, "not a PNG file")
        info, image = parsed[0], None
        if info is not None and (info["height"], info["width"]) == tuple(shape) and info["channels"] != 4 and not info.get("palette", False):
            image = ops.png_decode_batch([data], device=self.device, reject_ok=True, parsed=[parsed], kinds=("colour", "mask"))[0]
        self.stats["mask_fallbacks" if image is None else "masks_decoded_on_device"] += 1
        return None if image is None else ops.mask_place(image, mode="bgr_f32")

    def _decode_png(self, got, into, channels):
        """a PNG file's image on the device, or None where the path refuses the file or gives it up (``png_fallbacks``)"""
        image = got.image if got.png_tried else self._png_decode([_PngRequest(got.data, channels, None, into)])[0]
        self.stats["png_fallbacks" if image is None else "png_decoded_on_device"] += 1
        return image

    def _decode_jpeg(self, data, into):
        """a JPEG stream's image on the device, or None where the path refuses the stream (``jpeg_fallbacks``)"""
        from .. import ops

        info, image = ops.jpeg_info(data), None
        if info is not None:
            out = self._slot_for(into, info["height"], info["width"])  # (a served stream has three channels)
            if self.device_entropy:  # the scan on the device too; the call waits for its status word
                image, on_device = ops.jpeg_decode_device(data, out=out, device=self.device, reject_ok=True)
                self.stats["scans_decoded_on_device" if on_device else "entropy_fallbacks"] += 1
            else:
                image = ops.jpeg_decode(data, out=out, device=self.device, reject_ok=True)
        if image is None:
            self.stats["jpeg_fallbacks"] += 1
        return image

    # ------------------------------------------------------------------ the resize on the device
    @staticmethod
    def _is_u8_rgb(image):
        """uint8 [H,W,3], a host array or a tensor on a GPU"""
        u8 = image.dtype == torch.uint8 and image.is_cuda if isinstance(image, torch.Tensor) else image.dtype == np.uint8
        return u8 and image.ndim == 3 and image.shape[2] == 3

    def _device_plan(self, image, shape, filter):
        """the plan of ``image`` -> ``shape`` where the device path serves it: uint8 [H,W,3] of a size that is not refused"""
        if not self.device_resize or not self._is_u8_rgb(image):
            return None
        from .. import ops

        return ops.resample_plan(image.shape[:2], shape, filter, self.device, reject_ok=True)

    def _upload(self, image):
        """the bytes on the device through pinned memory: an asynchronous copy, nothing waits; an image decoded there stays"""
        if isinstance(image, torch.Tensor):
            return image
        host = torch.empty(image.shape, dtype=torch.uint8, pin_memory=True)
        host.copy_(torch.from_numpy(np.ascontiguousarray(image)))
        return host.to(self.device, non_blocking=True)

    def serves_target(self, image, shape):
        """whether ``expand_target`` takes the image as decoded (else the caller makes the target with the host statements)"""
        return self.device_resize and (tuple(image.shape[:2]) == tuple(shape) and self._is_u8_rgb(image) or
                                       self._device_plan(image, shape, "box") is not None)

    def expand_target(self, image_u8, shape):
        """a target's bytes on the device, as decoded -> float32 [h,w,3] = BOX-resized to ``shape`` where the size differs, / 255"""
        from .. import ops

        if tuple(image_u8.shape[:2]) != tuple(shape):
            image_u8 = ops.resample_u8(image_u8, shape, "box")
            self.stats["targets_resized_on_device"] += 1
        return ops.item_target(image_u8)[0]

    def resize_stack(self, images, shape, filter):
        """``_common.resize(image, *shape, filter)`` of every image (host arrays in, host arrays out): images of one size that
        the device path serves go through one batched ``ops.resample_u8``, the others through the host statement"""
        from .. import ops

        resample = {"box": PIL.Image.Resampling.BOX, "lanczos": PIL.Image.Resampling.LANCZOS}[filter]
        out, batches = [None] * len(images), {}
        for i, im in enumerate(images):
            if tuple(im.shape[:2]) != tuple(shape) and self._device_plan(im, shape, filter) is not None:
                batches.setdefault(im.shape, []).append(i)
            else:
                out[i] = resize(im, *shape, resample)
        for idx in batches.values():
            got = ops.resample_u8(self._upload(np.stack([images[i] for i in idx])), shape, filter).cpu().numpy()
            self.stats["frames_resized_on_device"] += len(idx)
            for i, g in zip(idx, got):
                out[i] = g
        return out

    def put(self, scene, f, rgb, mask, depth, scale_shift=None, zoe_pair=None):
        """a decoded frame (image uint8 [H,W,3], mask bool or uint8 [H,W], depth [H,W]) into the slot of frame id ``f``.  With
        ``device_resize`` the image may come at the file's size: it is BOX-resized into the slot on the device; with
        ``device_decode`` it may be on the device already (``decode_image``), and may be the slot itself.  A scene in
        prediction mode takes ``depth`` = the float32 ``depth_pred`` with ``scale_shift`` = the file's (scale, shift), float64,
        and (optionally) the pair they belong to"""
        shape = (scene.h, scene.w)
        (slot,) = self.slots(scene, [f])
        plan = None
        if self.device_resize and tuple(rgb.shape[:2]) != shape:
            plan = self._device_plan(rgb, shape, "box")
            if plan is None:
                if isinstance(rgb, torch.Tensor):  # (a size the device resize refuses: back to the host, which waits)
                    rgb = rgb.cpu().numpy()
                rgb = resize(rgb, *shape, PIL.Image.Resampling.BOX)  # the host statement
        if plan is None and (not self._is_u8_rgb(rgb) or tuple(rgb.shape) != shape + (3,)):
            raise ValueError(f"frame {f}: image {rgb.dtype} {rgb.shape}, the store keeps uint8 {shape + (3,)}")
        if mask.dtype not in (np.bool_, np.uint8, torch.uint8) or tuple(mask.shape) != shape:
            raise ValueError(f"frame {f}: mask {mask.dtype} {tuple(mask.shape)}, the store keeps bool or uint8 {shape}")
        if tuple(depth.shape) != shape or (isinstance(depth, torch.Tensor) and depth.dtype != torch.float32):
            raise ValueError(f"frame {f}: depth {depth.dtype} {tuple(depth.shape)}, expected {shape} (a tensor: float32)")
        if scene.prediction != (scale_shift is not None):
            raise ValueError(f"frame {f}: a scene in prediction mode takes a prediction with its scale and shift, any other scene a depth alone")
        if scene.prediction:
            scale, shift = (np.asarray(x) for x in scale_shift)
            if depth.dtype not in (np.float32, torch.float32) or scale.dtype != np.float64 or shift.dtype != np.float64 or scale.ndim or shift.ndim:
                raise ValueError(f"frame {f}: depth_pred {depth.dtype}, scale {scale.dtype} {scale.shape}, shift {shift.dtype} {shift.shape}; "
                                 "the store keeps float32 predictions and 0-d float64 scales and shifts")
            scene.scale_shift[slot] = (scale, shift)
            scene.zoe_pairs[slot] = zoe_pair
        if plan is not None:
            from .. import ops

            ops.resample_u8(self._upload(rgb), shape, "box", out=scene.rgb[slot])
            self.stats["frames_resized_on_device"] += 1
        elif isinstance(rgb, torch.Tensor):
            if rgb.data_ptr() != scene.rgb[slot].data_ptr():  # (else decode_image wrote the slot)
                scene.rgb[slot].copy_(rgb)
        else:
            scene.rgb[slot].copy_(torch.from_numpy(np.ascontiguousarray(rgb)))
        if isinstance(mask, torch.Tensor):
            if mask.data_ptr() != scene.dyn_mask[slot].data_ptr():  # (else decode_mask wrote the slot)
                scene.dyn_mask[slot].copy_(mask)
        else:
            scene.dyn_mask[slot].copy_(torch.from_numpy(np.ascontiguousarray(mask, dtype=np.uint8)))
        if isinstance(depth, torch.Tensor):
            if depth.data_ptr() != scene.depth[slot].data_ptr():  # (else _fill's depth_place wrote the slot)
                scene.depth[slot].copy_(depth)
        else:
            scene.depth[slot].copy_(F32(depth))
        scene.filled[slot] = True
        self.stats["frames_decoded"] += 1

    def views(self, scene, groups, decode, image_path=None, mask_path=None, *, depth_request=None):
        """one dict per group ``(frame ids, with_depth)``: rgb, dyn_rgb, static_rgb [n,H,W,3], dyn_mask and (with_depth) depth
        [n,H,W,1], float32 on the store's device; ``decode(frame id) -> (rgb uint8, mask, depth)`` fills missing slots;
        ``image_path(frame id)`` -> the frame's image file (or (file, channels)): with ``device_png`` the missing frames'
        files are prefetched in one launch; ``mask_path(frame id)`` -> the frame's mask file: with ``device_mask`` in the same one;
        ``depth_request(frame id)`` -> the frame's depth file and statement (``_stage_depths``): with ``device_depth`` the missing
        frames' depths are placed in one launch"""
        frame_ids = [int(f) for ids, _ in groups for f in ids]
        groups = [(self.slots(scene, ids), with_depth) for ids, with_depth in groups]  # (checked before anything is decoded)
        self._fill(scene, frame_ids, decode, image_path, **({"mask_path": mask_path} if self.device_mask and mask_path is not None else {}),
                   **({"depth_request": depth_request} if self.device_depth and depth_request is not None else {}))
        if scene.prediction and any(with_depth for _, with_depth in groups):
            raise ValueError("a scene in prediction mode holds no depths: zoe_depths aligns its predictions")
        self.stats["items_built"] += 1
        if self.device is not None:
            from .. import ops

            return ops.item_views(scene.rgb, scene.dyn_mask, scene.depth, groups)
        out = []
        for ids, with_depth in groups:
            idx = torch.as_tensor(list(ids), dtype=torch.int64)
            rgb = scene.rgb[idx].numpy().astype(np.float32) / 255.0  # the disk path's statements, on the gathered stack
            mask = scene.dyn_mask[idx].numpy().astype(np.float32)
            o = {"rgb": F32(rgb), "dyn_rgb": F32(rgb * mask[..., None]), "static_rgb": F32(rgb * (1 - mask[..., None])),
                 "dyn_mask": F32(mask)[..., None]}
            if with_depth:
                o["depth"] = scene.depth[idx][..., None]
            out.append(o)
        return out

    def zoe_depths(self, scene, ids_by_group, range_cams=None, rays=None, c2w_tgt=None):
        """the aligned ZoeDepth depths of a scene in prediction mode, its slots filled (``views`` fills them): ([depth float32
        [n,H,W,1] per group], depth_range float32 [2] or None) on the store's device.  The range is taken over the FIRST
        group (the spatial one) seen from ``c2w_tgt``, on a host store with ``range_cams`` = (K [n,4,4], c2w [n,4,4]) through
        the disk path's statements (``zoe_align`` with the stored 0-d float64 scale and shift, ``spatial_depth_range``: they
        follow the installed NumPy as that path does), on a GPU store with ``rays`` [n,12] on the device through
        ``ops.item_zoe_depth``, which pins NumPy 2's result as ``ops.nvidia_zoe_depth`` does and waits for nothing"""
        from . import nvidia_eval as NE

        assert scene.prediction, "zoe_depths serves a scene opened in prediction mode"
        slots = [self.slots(scene, ids) for ids in ids_by_group]
        flat = [s for g in slots for s in g]
        assert scene.filled[flat].all(), "zoe_depths: views() fills the slots first"
        if self.device is not None:
            from .. import ops

            inv = None if rays is None else np.linalg.inv(c2w_tgt)
            return ops.item_zoe_depth(scene.depth, slots, scene.scale_shift[flat], rays, inv)
        depths = [np.stack([NE.zoe_align(scene.depth[s].numpy(), np.asarray(scene.scale_shift[s, 0]), np.asarray(scene.scale_shift[s, 1]))
                            for s in g]) for g in slots]
        rng = None
        if range_cams is not None:
            rng = NE.spatial_depth_range({"depth": depths[0], "K": range_cams[0], "c2w": range_cams[1]}, c2w_tgt,
                                         f64_depth=depths[0].dtype == np.float64)
        return [F32(d)[..., None] for d in depths], rng

    # ------------------------------------------------------------------ flow pairs
    def flow(self, scene, a, b, path):
        """(flow [H,W,2], occlusion mask [H,W,1]) of the pair, fresh tensors on the store's device; ``path`` None is the
        placeholder pair (a frame with itself): zeros"""
        dev = self.device if self.device is not None else "cpu"
        if path is None:
            return (torch.zeros((scene.h, scene.w, 2), dtype=torch.float32, device=dev),
                    torch.zeros((scene.h, scene.w, 1), dtype=torch.float32, device=dev))
        pair = scene.flows.get((a, b))
        if pair is None:
            pair = scene.flows[a, b] = self._read_flow(scene, path)
            while self.nbytes > self.resident_max_bytes and self._drop_flow_pair(keep=(scene, (a, b))):
                pass
            if self.nbytes > self.resident_max_bytes:  # no room for even this pair: it serves this item and is not kept
                del scene.flows[a, b]
        else:
            scene.flows.move_to_end((a, b))
        return pair[0].clone(), pair[1].clone()[..., None]

    def _upload_flow_pair(self, scene, path):
        """``device_depth``: (flow, coord_diff) float32 [H,W,2] on the device, views of ONE uploaded buffer that holds both payloads
        as the file stores them -- where both are stored ``<f4`` members of the scene's size; else None: ``_read_flow``'s own
        statement reads the file, errors included.  The pair's flow keeps the buffer (``_pair_bytes`` counts it)."""
        from . import npy_file

        with open(path, "rb") as f:
            data = f.read()
        spans = [npy_file.npz_member(data, name)[:2] for name in ("flow", "coord_diff")]
        if any(offset is None or tuple(shape) != (scene.h, scene.w, 2) for offset, shape in spans):
            return None
        nbytes = scene.h * scene.w * 8
        host = torch.empty(2 * _pad16(nbytes), dtype=torch.uint8, pin_memory=True)
        for k, (offset, _) in enumerate(spans):
            host.numpy()[k * _pad16(nbytes):k * _pad16(nbytes) + nbytes] = np.frombuffer(data, np.uint8, nbytes, offset)
        dev = host.to(self.device, non_blocking=True)
        return tuple(dev[k * _pad16(nbytes):k * _pad16(nbytes) + nbytes].view(torch.float32).view(scene.h, scene.w, 2) for k in range(2))

    def _read_flow(self, scene, path):
        self.stats["flow_files_read"] += 1
        if self.device is None:
            flow, occ = read_flow_npz(path, self.occ_thres)
            assert flow.shape[:2] == (scene.h, scene.w), (flow.shape, (scene.h, scene.w))
            return F32(flow), F32(occ)
        from .. import ops

        if self.device_depth:  # the file read once, both members as stored in one pinned buffer, one asynchronous copy
            pair = self._upload_flow_pair(scene, path)
            if pair is not None:
                return pair[0], ops.flow_occ(pair[1], self.occ_thres)
        info = np.load(path)
        flow, cd = info["flow"], info["coord_diff"]
        assert flow.shape[:2] == (scene.h, scene.w), (flow.shape, (scene.h, scene.w))
        if cd.dtype != np.float32:
            raise ValueError(f"{path}: coord_diff is {cd.dtype}; ops.flow_occ states the float32 files' sum and compare")
        return F32(flow).to(self.device), ops.flow_occ(torch.from_numpy(np.ascontiguousarray(cd)).to(self.device), self.occ_thres)


# ---------------------------------------------------------------------------- items
def pack_to_device(entries, device):
    """the host tensors of ``entries`` on ``device`` through ONE pinned buffer and one asynchronous copy: each entry becomes a
    view of the uploaded bytes at a 16-byte boundary (entries are disjoint; nothing else refers to the buffer); an entry that
    is on a GPU already is handed through as it is"""
    there = {k: t for k, t in entries.items() if t.is_cuda}  # (e.g. a target image decoded on the device)
    entries = {k: t for k, t in entries.items() if not t.is_cuda}
    offs, total = {}, 0
    for k, t in entries.items():
        offs[k] = total
        total += _pad16(t.numel() * t.element_size())
    host = torch.empty(max(total, 16), dtype=torch.uint8, pin_memory=True)
    for k, t in entries.items():
        n = t.numel() * t.element_size()
        host[offs[k]:offs[k] + n].copy_(t.contiguous().view(-1).view(torch.uint8))
    dev = host.to(device, non_blocking=True)
    out = {k: dev[offs[k]:offs[k] + t.numel() * t.element_size()].view(t.dtype).view(t.shape) for k, t in entries.items()}
    out.update(there)
    return out


def group_host_entries(group, flat_cams, times=None, n_actual=None):
    """the host-made entries of one group, as ``_common.group_entries`` makes them"""
    out = {f"flat_cam_src_{group}": F32(flat_cams)}
    if times is not None:
        out[f"time_src_{group}"] = torch.FloatTensor(times)
    if n_actual is not None:
        out[f"n_actual_{group}"] = torch.LongTensor([n_actual])
    return out


def build_item(store, scene, decode, *, fixed, host, cams, sel, spatial_ids, spatial_depth, c2w_tgt, flow_path, trackers, owner,
               ray_rows=None, depth_range=None, depths=None, image_path=None, mask_path=None, depth_request=None):
    """An item of the five loaders from the store, key for key and bit for bit the disk path's.  ``fixed``: the
    non-tensor entries; ``host``: the host-made tensors (on a GPU store they travel in ONE packed copy, with the groups'
    cameras and times; entries named ``__...`` are the loader's own cargo: they come back in the item, on the device, for
    the loader to take out); ``cams(frame ids) -> (flat_cam [V,34], K [V,4,4], c2w [V,4,4])``; ``sel``: the loader's temporal
    selection; ``spatial_ids`` (None: no spatial group and no ``depth_range``) with ``spatial_depth`` False where the item
    carries no spatial depth (the range is still taken over it); ``flow_path(a, b)``: the pair's file, None for the
    placeholder pair.  ``depth_range``: ``nvidia_eval.spatial_depth_range`` on the host, ``ops.nvidia_depth_range`` on the
    gathered depths on a GPU store, where nothing here waits for the device.  The DyCheck loader brings its own:
    ``ray_rows(spatial ids) -> [V,12] float32`` (its cached ray constants; default: ``nvidia_eval.ray_rows`` of the cameras,
    formed on a GPU store only) and ``depth_range(depth [V,H,W], dyn_mask [V,H,W], rays) -> tensor`` on the store's device,
    ``rays`` the rows as a device tensor on a GPU store and as the numpy array on a host store; ``c2w_tgt`` is unused then.
    The NVIDIA evaluation loader's ZoeDepth inputs bring ``depths(ids per group, (K, c2w) of the spatial group or None, rays or
    None) -> ([depth [n,H,W,1] per group], depth_range or None)`` on the store's device (``SceneStore.zoe_depths`` over a
    scene in prediction mode): the store then gathers colours and masks alone, and every depth and the range come from there.
    ``image_path(frame id)``: the frame's image file, for ``SceneStore.views`` to prefetch under ``device_png``;
    ``mask_path(frame id)``: its mask file, for the same batch under ``device_mask``; ``depth_request(frame id)``: its depth file
    and the loader's statement over it (``SceneStore._stage_depths``), for the fill's one ``ops.depth_place`` under ``device_depth``."""
    from . import nvidia_eval as NE

    dev = store.device
    if dev is not None:
        NE.refuse_gpu_in_worker(owner)
    host, groups, rng, rows = dict(host), [], None, None

    def add(name, ids, with_depth, times=None, n_actual=None):
        flat, Ks, c2ws = cams(ids)
        host.update(group_host_entries(name, flat, times, n_actual))
        groups.append((name, [int(i) for i in ids], with_depth))
        return Ks, c2ws

    if spatial_ids is not None:
        rng = add("spatial", spatial_ids, spatial_depth)
        if ray_rows is not None:
            rows = np.ascontiguousarray(ray_rows(spatial_ids), dtype=np.float32)
        elif dev is not None:
            rows = NE.ray_rows(*rng)
        if dev is not None:
            host["__rays"] = F32(rows)
    add("temporal", sel["temporal"], True, sel["temporal"], sel["n_actual_temporal"])
    if trackers:
        for side in ("fwd2tgt", "bwd2tgt"):
            add(f"temporal_track_{side}", sel[side], True, sel[side], sel[f"n_actual_{side}"])
    # the range needs the spatial depths even where the item carries none (the visualisation loaders)
    views = store.views(scene, [(ids, depths is None and (with_depth or name == "spatial")) for name, ids, with_depth in groups], decode, image_path,
                        mask_path, **({"depth_request": depth_request} if store.device_depth and depth_request is not None else {}))
    small = pack_to_device(host, dev) if dev is not None else host
    rays = small.pop("__rays", None)
    item = dict(fixed)
    item.update(small)
    if depths is not None:
        aligned, zoe_range = depths([ids for _, ids, _ in groups], rng, rays)
        for v, d in zip(views, aligned):
            v["depth"] = d
        if spatial_ids is not None:
            item["depth_range"] = zoe_range
    for (name, _, with_depth), v in zip(groups, views):
        if name == "spatial" and depths is None:
            depth = v["depth"][..., 0]
            if depth_range is not None:
                item["depth_range"] = depth_range(depth, v["dyn_mask"][..., 0], rays if dev is not None else rows)
            elif dev is not None:
                from .. import ops

                item["depth_range"] = ops.nvidia_depth_range(depth, rays, np.linalg.inv(c2w_tgt))
            else:
                item["depth_range"] = NE.spatial_depth_range({"depth": depth.numpy(), "K": rng[0], "c2w": rng[1]}, c2w_tgt)
        item.update({f"{k}_src_{name}": v[k] for k in VIEW_KEYS if k != "depth" or with_depth})
    a, b = sel["temporal"]
    for key, (x, y) in (("fwd", (a, b)), ("bwd", (b, a))):
        item[f"flow_{key}"], item[f"flow_{key}_occ_mask"] = store.flow(scene, x, y, flow_path(x, y))
    return item
