"""Device-resident image tables: the factor datasets' images stay in HBM as uint8 and "look up these images" is one
kernel launch (``itcv_gather_u8``, csrc/dataset.hip).

The reference's factor datasets (dataset.py:40-201: dSprites 737 280 x 64 x 64 = 3.0 GB, MPI3D-toy 1 036 800 x 64 x 64 x 3
= 12.7 GB) are uint8 arrays in host memory, and every image an evaluation or a training step uses goes through
``__getitem__``: ``Image.fromarray`` + ``ToTensor`` (dataset.py:75-81,141-147), one Python call per image, then a pageable
host-to-device copy per batch.  A default FactorVAE score looks up 0.97 M images that way and a beta-VAE score 2.56 M.
Both tables fit in HBM many times over.  Here

  * ``DeviceImageTable`` holds the planar ``[N, C, H, W]`` uint8 table (and the label table) on the device;
    ``gather(idx)`` returns ``table[idx] / 255`` as fp32 -- ``ToTensor``'s ``.float().div(255)`` bit for bit;
  * ``DeviceFactorSampler`` is ``disentangle.FactorSampler`` with the image lookup replaced by one gather: same draws,
    same factors, same observations, so every ``compute_*`` score runs on it unchanged;
  * ``DeviceLoader`` feeds training from the table: one gather (+ flips) and one label ``index_select`` per batch;
  * ``DevicePairLoader`` feeds the weakly-supervised pair objective (solvers/ada.py): pairs of images that differ in a
    few factors, drawn on the device (``pair_factors``) and looked up with two gathers into one ``[2B, C, H, W]`` batch;
  * ``DeviceLabelledLoader`` feeds the semi-supervised S2 objectives (solvers/semi.py): unlabelled rows from an epoch
    permutation plus a few rows of a fixed labelled subset, with their integer factor values (``index_factors``).

Datasets that resize (``resize != H``: ``Image.resize(..., Image.BICUBIC)`` per sample, dataset.py:78-79,144-145,335) run
that resize on the device too, bit for bit (``itcv_resize_u8``, csrc/resize.hip, with the plans of hipvae/resize.py):
either once, into a second table (``resized``), or inside every lookup (``view_resized``, when the resized table would not
fit).  ``from_dataset(..., device_resize="table" | "gather" | "auto")`` chooses; without the keyword such a dataset is
refused as before.  Decoding image files (UkiyoE's JPEGs) stays a host job, done once per table
(``from_image_files``).

Everything is opt-in (``VAESolver.use_device_dataset``); nothing here is used unless asked for.
"""
import os

import numpy as np
import torch

from . import abi
from .disentangle import FactorSampler
from .resize import ResizePlan

__all__ = ["DeviceImageTable", "ResizedView", "DeviceFactorSampler", "DeviceLoader", "DevicePairLoader", "pair_factors",
           "factor_bases", "DeviceLabelledLoader", "index_factors"]

UPLOAD_CHUNK_BYTES = 256 << 20
RESIZE_MODES = (None, "table", "gather", "auto")
FILE_INPUT_HEIGHT = 256         # UkiyoE.__getitem__ (dataset.py:232-238): load_image(..., input_height=256, ...)


def _device(device):
    return torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())


def _size_pair(size):
    """``(Hout, Wout)`` of a ``size`` given as one int (square, as the reference's ``resize``) or as a pair."""
    pair = tuple(size) if isinstance(size, (tuple, list)) else (size, size)
    if len(pair) != 2 or not all(isinstance(v, (int, np.integer)) and v >= 1 for v in pair):
        raise ValueError(f"resize: the size must be a positive int or a pair of them, got {size!r}")
    return int(pair[0]), int(pair[1])


class DeviceImageTable:
    """A planar uint8 image table ``[N, C, H, W]`` in device memory, with an optional label table ``[N, ...]``."""

    def __init__(self, images, labels=None):
        if not isinstance(images, torch.Tensor) or images.dtype != torch.uint8 or images.dim() != 4:
            raise TypeError("DeviceImageTable needs a uint8 tensor [N, C, H, W]")
        if not images.is_contiguous():
            raise ValueError("DeviceImageTable needs a contiguous (planar) tensor")
        if images.shape[0] < 1 or images[0].numel() < 1 or images[0].numel() >= 1 << 31:
            raise ValueError(f"DeviceImageTable: unsupported table shape {tuple(images.shape)}")
        if labels is not None and labels.shape[0] != images.shape[0]:
            raise ValueError("DeviceImageTable: one label row per image")
        self.images, self.label_table = images, labels
        self.num_images, self.image_shape = int(images.shape[0]), tuple(int(s) for s in images.shape[1:])
        self.device = images.device
        self.factor_sizes = self.latent_indices = None      # set by from_dataset for a dataset ordered by its factors
        self._flags = None

    def __len__(self):
        return self.num_images

    # ---- construction ------------------------------------------------------------------------------------------------
    @classmethod
    def from_device_tensor(cls, u8, labels=None):
        """The table IS ``u8`` (planar ``[N, C, H, W]`` uint8 on the device); nothing is copied."""
        if not (isinstance(u8, torch.Tensor) and u8.is_cuda):
            raise abi.HipExtensionError("from_device_tensor needs a device tensor; there is no CPU path")
        return cls(u8, labels)

    @classmethod
    def from_arrays(cls, images_u8, labels=None, device=None):
        """Upload ``[N, H, W]`` or ``[N, H, W, C]`` numpy uint8 images in chunks of at most 256 MiB; an HWC chunk is
        turned planar once, on the device.  Raises ``MemoryError`` when the device does not have the room."""
        images_u8 = cls._check_arrays(images_u8)
        device = _device(device)
        N, H, W = images_u8.shape[:3]
        C = images_u8.shape[3] if images_u8.ndim == 4 else 1
        per_image = C * H * W
        rows = max(1, min(N, UPLOAD_CHUNK_BYTES // per_image))
        lab = None if labels is None else np.ascontiguousarray(labels)
        need = N * per_image + rows * per_image + (0 if lab is None else lab.nbytes)
        free, _ = torch.cuda.mem_get_info(device)
        if need > free:
            raise MemoryError(f"DeviceImageTable: the table needs {need} bytes of device memory, {free} are free")
        table = torch.empty((N, C, H, W), dtype=torch.uint8, device=device)
        for a in range(0, N, rows):
            chunk = torch.from_numpy(np.ascontiguousarray(images_u8[a:a + rows])).to(device)
            dst = table[a:a + rows]
            dst.copy_(chunk.permute(0, 3, 1, 2) if chunk.dim() == 4 else chunk.unsqueeze(1))
        return cls(table, None if lab is None else torch.from_numpy(lab).to(device))

    @staticmethod
    def _check_arrays(images_u8):
        images_u8 = np.asarray(images_u8)
        if images_u8.dtype != np.uint8:
            raise TypeError(f"DeviceImageTable needs uint8 images, got {images_u8.dtype}")
        if images_u8.ndim not in (3, 4) or images_u8.shape[0] < 1:
            raise ValueError(f"DeviceImageTable needs images [N, H, W] or [N, H, W, C], got {images_u8.shape}")
        return images_u8

    @classmethod
    def from_dataset(cls, ds, device=None, device_resize=None):
        """The table of a reference factor dataset (dataset.py:40-201): ``ds.imgs`` exactly as the class stored it -- the
        ``* 255`` of its constructor included, which wraps modulo 256 on uint8 -- and ``ds.latents_values`` as labels.
        Refuses, before touching the device, what ``__getitem__`` would not turn into ``imgs[i] / 255``: images that are
        not uint8 (``TypeError``) and, unless ``device_resize`` opts in, a ``resize`` other than the stored height
        (``NotImplementedError``).

        ``device_resize`` -- how a dataset that resizes is served: ``"table"`` resizes the whole table once on the device
        (``resized``), ``"gather"`` keeps the stored size and resizes inside every lookup (``view_resized``), ``"auto"``
        takes the table when it fits in free device memory next to the source table and the view otherwise; anything
        else is a ``ValueError``.  With it, a file-backed dataset (``root``, ``entries`` of (file name, label code) and
        ``resize``, no ``imgs``: UkiyoE) is accepted too: its files are decoded once on the host (``from_image_files``)
        and its label codes become the label table."""
        if device_resize not in RESIZE_MODES:
            raise ValueError(f"from_dataset: device_resize must be one of {RESIZE_MODES}, got {device_resize!r}")
        resize = getattr(ds, "resize", None)
        if not hasattr(ds, "imgs") and all(hasattr(ds, a) for a in ("root", "entries", "resize")):
            if device_resize is None:
                raise NotImplementedError("from_dataset: a dataset that decodes files needs device_resize= (the files are "
                                          "then decoded once, on the host)")
            entries = list(ds.entries)
            table = cls.from_image_files([os.path.join(ds.root, e[0]) for e in entries],
                                         np.array([e[1] for e in entries]), FILE_INPUT_HEIGHT, None, device)
        else:
            imgs = np.asarray(ds.imgs)
            if imgs.dtype != np.uint8:
                raise TypeError(f"from_dataset: {type(ds).__name__}.imgs is {imgs.dtype}, not uint8")
            imgs = cls._check_arrays(imgs)
            if resize is not None and int(resize) != imgs.shape[1] and device_resize is None:
                raise NotImplementedError(f"from_dataset: resize={resize} differs from the stored height "
                                          f"{imgs.shape[1]}; pass device_resize= to resize on the device")
            table = cls.from_arrays(imgs, getattr(ds, "latents_values", None), device)
        try:        # the base class's properties raise NotImplementedError; a plain image dataset has neither
            table.factor_sizes, table.latent_indices = list(ds.factor_sizes), list(ds.latent_indices)
        except (AttributeError, NotImplementedError):
            table.factor_sizes = table.latent_indices = None
        if device_resize is None or resize is None or (int(resize), int(resize)) == table.image_shape[1:]:
            return table
        if device_resize == "gather":
            return table.view_resized(int(resize))
        try:
            return table.resized(int(resize))
        except MemoryError:
            if device_resize != "auto":
                raise
            return table.view_resized(int(resize))

    @staticmethod
    def decode_image_files(paths, input_height=FILE_INPUT_HEIGHT):
        """The host half of ``from_image_files``: uint8 ``[N, input_height, input_height, 3]``, every file decoded once
        as ``load_image`` (dataset.py:310-320) does before its last line: ``Image.open``, ``convert("RGB")`` unless
        already RGB, ``resize((input_height, input_height), Image.BICUBIC)`` (which returns a same-size image
        unchanged)."""
        from PIL import Image
        paths = list(paths)
        if not paths:
            raise ValueError("decode_image_files: no files")
        out = np.empty((len(paths), input_height, input_height, 3), dtype=np.uint8)
        for i, path in enumerate(paths):
            with Image.open(path) as img:
                if img.mode != "RGB":
                    img = img.convert("RGB")
                out[i] = np.asarray(img.resize((input_height, input_height), Image.BICUBIC))
        return out

    @classmethod
    def from_image_files(cls, paths, labels=None, input_height=FILE_INPUT_HEIGHT, resize=None, device=None):
        """The table of a dataset of image files (UkiyoE, dataset.py:207-240): ``decode_image_files`` on the host, one
        upload of the ``[N, 3, input_height, input_height]`` table, and ``load_image``'s last line -- the resize to
        ``resize`` -- on the device (``resized``) when it changes the size.  ``DeviceLoader(table, B, flip_p=0.5)`` is then
        the dataset's ``RandomHorizontalFlip`` (resize first, mirror after, as the reference)."""
        table = cls.from_arrays(cls.decode_image_files(paths, input_height), labels, device)
        return table if resize is None else table.resized(resize)

    # ---- resize ------------------------------------------------------------------------------------------------------
    def _carry(self, other):
        other.label_table, other.factor_sizes, other.latent_indices = self.label_table, self.factor_sizes, self.latent_indices
        return other

    def resized(self, size):
        """A new materialised uint8 table ``[N, C, Hout, Wout]``: every image through Pillow's bicubic resize, bit for bit
        (``itcv_resize_u8``, in chunks of at most 256 MiB of output); labels and factor structure are carried over.
        ``size``: an int (square) or ``(Hout, Wout)``; the table itself when nothing changes.  Raises ``MemoryError`` when
        the device does not have the room."""
        Hout, Wout = _size_pair(size)
        C, H, W = self.image_shape
        if (Hout, Wout) == (H, W):
            return self
        N, per_image = self.num_images, C * Hout * Wout
        free, _ = torch.cuda.mem_get_info(self.device)
        if N * per_image > free:
            raise MemoryError(f"DeviceImageTable: the resized table needs {N * per_image} bytes of device memory, "
                              f"{free} are free")
        plan = ResizePlan.get(H, W, Hout, Wout, self.device)
        out = torch.empty((N, C, Hout, Wout), dtype=torch.uint8, device=self.device)
        flags = torch.zeros(1, dtype=torch.int32, device=self.device)
        rows = max(1, min(N, UPLOAD_CHUNK_BYTES // per_image))
        for a in range(0, N, rows):
            n = min(rows, N - a)
            plan.launch(self.images[a:a + n], n, C, None, n, None, out[a:a + n], flags)
        if flags.item():
            raise RuntimeError(f"resized: the {H}x{W} -> {Hout}x{Wout} plan was refused by the kernel")
        return self._carry(DeviceImageTable(out))

    def view_resized(self, size):
        """A table object over the SAME ``images`` whose ``image_shape`` is ``(C, Hout, Wout)`` and whose ``gather``
        resizes inside the lookup: what ``resized(size).gather`` returns, bit for bit, without the second table."""
        Hout, Wout = _size_pair(size)
        if (Hout, Wout) == self.image_shape[1:]:
            return self
        return self._carry(ResizedView(self, Hout, Wout))

    # ---- lookup ------------------------------------------------------------------------------------------------------
    def _index(self, idx):
        """``(int64 device tensor [n], came from the host)``; host indices are range-checked here, before any launch."""
        if isinstance(idx, torch.Tensor) and idx.is_cuda:
            if idx.dtype != torch.int64 or idx.dim() != 1:
                raise TypeError("device indices must be a 1-D int64 tensor")
            return idx.contiguous(), False
        host = np.asarray(idx.cpu() if isinstance(idx, torch.Tensor) else idx)
        if host.ndim != 1 or (host.size and host.dtype.kind not in "iu"):
            raise TypeError("indices must be a 1-D integer array")
        host = host.astype(np.int64)
        if host.size and (host.min() < 0 or host.max() >= self.num_images):
            bad = host[(host < 0) | (host >= self.num_images)][0]
            raise IndexError(f"image index {int(bad)} is outside [0, {self.num_images})")
        return torch.from_numpy(host).to(self.device), True

    def gather(self, idx, out=None, flip=None, check=True):
        """fp32 ``[n, C, H, W]``: ``table[idx] / 255``, image j mirrored along W where ``flip[j] != 0``.  ``idx``: a numpy
        array / list (range-checked on the host: ``IndexError``, nothing launched) or an int64 device tensor (an index
        outside the table yields a zero image and raises the table's flag, which is read back -- one synchronisation --
        when ``check`` is true and otherwise by ``check()``).  ``out``: a dense fp32 ``[n, C, H, W]`` device tensor to
        write, e.g. a row slice of a larger preallocated buffer."""
        idx, from_host = self._index(idx)
        n = idx.shape[0]
        shape = (n,) + self.image_shape
        if out is None:
            out = torch.empty(shape, dtype=torch.float32, device=self.device)
        elif tuple(out.shape) != shape or out.dtype != torch.float32 or out.device != self.device:
            raise ValueError(f"gather: out must be a float32 {shape} tensor on {self.device}")
        if n == 0:
            return out
        if flip is not None:
            flip = torch.as_tensor(np.asarray(flip) if not isinstance(flip, torch.Tensor) else flip)
            flip = flip.to(device=self.device, dtype=torch.uint8)
            if flip.shape != (n,):
                raise ValueError("gather: one flip flag per index")
        if self._flags is None:
            self._flags = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._launch_gather(idx, n, flip, out)
        if check and not from_host:
            self.check()
        return out

    def _launch_gather(self, idx, n, flip, out):
        C, H, W = self.image_shape
        abi.call("itcv_gather_u8", abi.ptr(self.images), self.num_images, C * H, W, abi.ptr(idx), n, abi.ptr(flip),
                 abi.ptr(out), self._flags.data_ptr(), abi.stream())

    def check(self):
        """Read the out-of-range flag of the gathers since the last check (one synchronisation); raises ``IndexError``."""
        bits = self._flags.item() if self._flags is not None else 0
        if bits:
            self._flags.zero_()
            if bits & 2:
                raise RuntimeError("a resize plan was refused by the kernel; the images were returned as zeros")
            raise IndexError(f"a device index was outside [0, {self.num_images}); its image was returned as zeros")

    def labels(self, idx):
        """Rows ``idx`` of the label table (torch ``index_select``)."""
        if self.label_table is None:
            raise ValueError("this table has no labels")
        return self.label_table.index_select(0, self._index(idx)[0])


class ResizedView(DeviceImageTable):
    """``DeviceImageTable.view_resized``: the source table's ``images`` under the resized ``image_shape``.  Everything a
    sampler or a loader uses (``gather``, ``labels``, ``check``, ``image_shape``, ``num_images``, ``label_table``,
    ``device``) behaves as on the materialised table; ``gather`` is the fused form of ``itcv_resize_u8``."""

    def __init__(self, source, Hout, Wout):
        self.images, self.num_images, self.device = source.images, source.num_images, source.device
        self.source_shape = source.image_shape
        self.image_shape = (source.image_shape[0], Hout, Wout)
        self.label_table = self.factor_sizes = self.latent_indices = None
        self._flags = None
        self._plan = None

    def _launch_gather(self, idx, n, flip, out):
        C, H, W = self.source_shape
        if self._plan is None:
            self._plan = ResizePlan.get(H, W, self.image_shape[1], self.image_shape[2], self.device)
        self._plan.launch(self.images, self.num_images, C, idx, n, flip, out, self._flags)

    def resized(self, size):
        raise ValueError("a resized view is not resized again: resize the source table")

    view_resized = resized


class DeviceFactorSampler(FactorSampler):
    """``FactorSampler`` whose observations come from a ``DeviceImageTable``: ``indices_from_factors`` (numpy, the same
    ``RandomState`` draws in the same order), one small host-to-device index copy, one gather.  With equal seeds it
    returns exactly ``FactorSampler``'s factors and observations.  ``dataset_or_table``: a dataset (its table is built
    with ``from_dataset(..., device_resize=device_resize)`` unless ``table`` is given) or a table that carries
    ``factor_sizes`` / ``latent_indices``."""

    def __init__(self, dataset_or_table, device, seed=None, table=None, device_resize=None):
        if isinstance(dataset_or_table, DeviceImageTable):
            table = dataset_or_table
            if table.factor_sizes is None:
                raise ValueError("DeviceFactorSampler: the table carries no factor_sizes / latent_indices")
        elif table is None:
            table = DeviceImageTable.from_dataset(dataset_or_table, device, device_resize=device_resize)
        super().__init__(dataset_or_table, device, seed)
        total = int(np.prod(self.factor_sizes, dtype=np.int64))
        if total != table.num_images:
            raise ValueError(f"DeviceFactorSampler: the factors index {total} images, the table holds {table.num_images}")
        self.table = table

    def sample_observations_from_factors(self, factors):
        return self.table.gather(self.indices_from_factors(factors))


class DeviceLoader:
    """Batches ``(x, y)`` straight from a ``DeviceImageTable``: ``len()`` and iteration as
    ``WrappedDataLoader(DataLoader(ds, batch_size, shuffle=True, drop_last=...), pre_process)`` (dataset.py:16-27,
    train.py:146-159), yielding ``pre_process(x, y)`` or ``(x, y)`` with ``x`` fp32 ``[B, C, H, W]`` on the device and
    ``y`` the rows of the label table (the image indices for a table without labels).

    The ORDER IS THIS CLASS'S OWN RULE, not torch's CPU sampler stream: every epoch draws one ``torch.randperm`` from a
    private device generator seeded with ``seed``, and with ``flip_p`` > 0 every batch draws its flip coins
    (``rand(B) < flip_p``; only the image is mirrored) from the same generator.  The same seed repeats the same epochs;
    torch's global RNG streams are untouched.  Everything runs on the current stream -- no side stream, hence no
    cross-stream reuse hazard -- and the table's index flag is checked once, at the end of the epoch."""

    def __init__(self, table_or_dataset, batch_size, device=None, shuffle=True, drop_last=False, seed=0, flip_p=0.0,
                 pre_process=None):
        if batch_size < 1:
            raise ValueError("batch_size must be positive")
        self.table = table_or_dataset if isinstance(table_or_dataset, DeviceImageTable) \
            else DeviceImageTable.from_dataset(table_or_dataset, device)
        self.batch_size, self.shuffle, self.drop_last = int(batch_size), bool(shuffle), bool(drop_last)
        self.flip_p, self.func, self.seed = float(flip_p), pre_process, int(seed)
        self._gen = None

    @staticmethod
    def batch_sizes(num_images, batch_size, drop_last=False):
        """The batch sizes of one epoch."""
        sizes = [batch_size] * (num_images // batch_size)
        if not drop_last and num_images % batch_size:
            sizes.append(num_images % batch_size)
        return sizes

    def __len__(self):
        return len(self.batch_sizes(self.table.num_images, self.batch_size, self.drop_last))

    def __iter__(self):
        t = self.table
        if self._gen is None:
            self._gen = torch.Generator(device=t.device).manual_seed(self.seed)
        order = torch.randperm(t.num_images, generator=self._gen, device=t.device) if self.shuffle \
            else torch.arange(t.num_images, device=t.device)
        row = 0
        for n in self.batch_sizes(t.num_images, self.batch_size, self.drop_last):
            idx = order[row:row + n]
            row += n
            flip = None
            if self.flip_p > 0.0:
                flip = (torch.rand(n, generator=self._gen, device=t.device) < self.flip_p).to(torch.uint8)
            x = t.gather(idx, flip=flip, check=False)
            y = t.label_table.index_select(0, idx) if t.label_table is not None else idx
            yield self.func(x, y) if self.func is not None else (x, y)
        t.check()


# ---- pairs for the weakly-supervised objective -------------------------------------------------------------------------
def factor_bases(factor_sizes):
    """Place value of every factor in the image index (the first factor most significant), as ``FactorSampler``'s."""
    sizes = [int(s) for s in factor_sizes]
    return [int(np.prod(sizes[i + 1:], dtype=np.int64)) for i in range(len(sizes))]


def _uniform_ints(sizes, rows, generator, device):
    """int64 ``[rows, len(sizes)]``, column j uniform in ``[0, sizes[j])``: ONE fp64 draw, scaled and floored."""
    sz = torch.tensor(sizes, dtype=torch.float64, device=device)
    u = torch.rand((rows, len(sizes)), dtype=torch.float64, generator=generator, device=device)
    return torch.minimum((u * sz).floor(), sz - 1).to(torch.int64)


def pair_factors(factor_sizes, latent_indices, batch_size, k=1, generator=None, device=None):
    """The factors of ``batch_size`` pairs of images as Locatello et al. (2020) draw them (disentanglement_lib's
    ``weak`` module): ``(first, second, changed)``, int64 ``[B, num_factors]`` twice and bool ``[B, num_latents]``.

      * ``first``: every factor uniform over its values -- the factors that do not vary included, which both images of a
        pair share;
      * per pair ``k`` latent factors chosen without replacement (``k = -1``: first a number uniform in
        ``1 .. num_latents - 1`` per pair); ``changed`` marks them, in the order of ``latent_indices``;
      * ``second``: ``first`` with the chosen factors drawn again, uniformly (a redrawn value may equal the old one, as in
        the library).

    Integer torch ops on ``device`` (any device) with the draws of ``generator`` in a fixed order: the first factors, the
    per-pair counts (``k = -1`` only), the choice, the redrawn values."""
    sizes, lat = [int(s) for s in factor_sizes], [int(i) for i in latent_indices]
    F, L, B = len(sizes), len(lat), int(batch_size)
    if B < 1:
        raise ValueError("batch_size must be positive")
    if not lat or len(set(lat)) != L or min(lat) < 0 or max(lat) >= F or min(sizes) < 1:
        raise ValueError(f"pair_factors: latent_indices {lat} do not name distinct factors of sizes {sizes}")
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not (k == -1 or 1 <= k <= L):
        raise ValueError(f"k must be -1 or in 1 .. {L}, the number of latent factors (got {k!r})")
    if k == -1 and L < 2:
        raise ValueError("k = -1 draws a number in 1 .. num_latents - 1: it needs at least two latent factors")
    first = _uniform_ints(sizes, B, generator, device)
    if k == -1:
        count = torch.randint(1, L, (B, 1), generator=generator, device=device)
    else:
        count = torch.full((B, 1), int(k), dtype=torch.int64, device=device)
    # the rank of an i.i.d. uniform score among its row: the `count` smallest are a uniform choice without replacement
    rank = torch.rand((B, L), generator=generator, device=device).argsort(dim=1).argsort(dim=1)
    changed = rank < count
    redrawn = _uniform_ints([sizes[i] for i in lat], B, generator, device)
    lat_t = torch.tensor(lat, dtype=torch.int64, device=device)
    second = first.clone()
    second[:, lat_t] = torch.where(changed, redrawn, first[:, lat_t])
    return first, second, changed


class DevicePairLoader:
    """Batches ``(x, changed)`` of image PAIRS from a ``DeviceImageTable`` that carries ``factor_sizes`` /
    ``latent_indices`` (any other table: ``ValueError``): ``x`` fp32 ``[2B, C, H, W]`` on the device, rows ``b`` and
    ``B + b`` a pair that differs in (at most) the ``k`` latent factors ``changed[b]`` marks (bool ``[B, num_latents]``);
    ``pre_process(x, changed)`` when given.  ``pair_factors`` draws the factors from a private device generator seeded
    with ``seed`` -- the same seed repeats the same epochs, torch's global RNG streams are untouched -- the table's bases
    turn both factor tuples into indices, and two gathers fill the halves of one buffer: no host round trip per image.
    ``factors`` holds the ``(first, second)`` factor tensors of the batch yielded last.  ``len()``: ``steps_per_epoch``,
    or ``num_images // (2 * batch_size)``.  The table's index flag is checked once, at the end of the epoch."""

    def __init__(self, table, batch_size, k=1, device=None, seed=0, steps_per_epoch=None, pre_process=None):
        if not isinstance(table, DeviceImageTable) or table.factor_sizes is None or table.latent_indices is None:
            raise ValueError("DevicePairLoader: the table carries no factor_sizes / latent_indices")
        total = int(np.prod(table.factor_sizes, dtype=np.int64))
        if total != table.num_images:
            raise ValueError(f"DevicePairLoader: the factors index {total} images, the table holds {table.num_images}")
        if device is not None and torch.device(device) != table.device:
            raise ValueError(f"DevicePairLoader: the table lives on {table.device}, not on {device}")
        if steps_per_epoch is not None and steps_per_epoch < 0:
            raise ValueError("steps_per_epoch must not be negative")
        # the remaining arguments are checked by the function that uses them (a throw-away host generator: the global
        # streams stay untouched), before the first batch
        pair_factors(table.factor_sizes, table.latent_indices, batch_size, k, torch.Generator(), "cpu")
        self.table, self.batch_size, self.k = table, int(batch_size), int(k)
        self.seed, self.steps_per_epoch, self.func = int(seed), steps_per_epoch, pre_process
        self.factors = None
        self._gen = self._bases = None

    def __len__(self):
        if self.steps_per_epoch is not None:
            return int(self.steps_per_epoch)
        return self.table.num_images // (2 * self.batch_size)

    def __iter__(self):
        t, B = self.table, self.batch_size
        if self._gen is None:
            self._gen = torch.Generator(device=t.device).manual_seed(self.seed)
            self._bases = torch.tensor(factor_bases(t.factor_sizes), dtype=torch.int64, device=t.device)
        for _ in range(len(self)):
            first, second, changed = pair_factors(t.factor_sizes, t.latent_indices, B, self.k, self._gen, t.device)
            x = torch.empty((2 * B,) + t.image_shape, dtype=torch.float32, device=t.device)
            t.gather((first * self._bases).sum(1), out=x[:B], check=False)
            t.gather((second * self._bases).sum(1), out=x[B:], check=False)
            self.factors = (first, second)
            yield self.func(x, changed) if self.func is not None else (x, changed)
        t.check()


# ---- a few labels for the semi-supervised objectives ---------------------------------------------------------------------
def index_factors(idx, factor_sizes, columns=None):
    """int64 ``[n, len(columns)]``: the factor values of the images ``idx`` (an int64 tensor on any device) of a table
    ordered by its factors, ``(idx // base_f) % size_f`` with ``factor_bases`` -- integers derived from the index, not the
    float ``latents_values`` of a label table.  ``columns`` None: every factor."""
    sizes = [int(s) for s in factor_sizes]
    cols = list(range(len(sizes))) if columns is None else [int(c) for c in columns]
    bases = torch.tensor([factor_bases(sizes)[c] for c in cols], dtype=torch.int64, device=idx.device)
    size_t = torch.tensor([sizes[c] for c in cols], dtype=torch.int64, device=idx.device)
    return (idx.reshape(-1, 1) // bases) % size_t


class DeviceLabelledLoader:
    """Batches ``(x, y)`` for the semi-supervised S2 solvers (solvers/semi.py) from a ``DeviceImageTable`` that carries
    ``factor_sizes`` / ``latent_indices`` (any other table: ``ValueError``): ``x`` fp32 ``[B + B_l, C, H, W]`` on the
    device whose first ``B`` rows are unlabelled and whose LAST ``B_l = labelled_batch_size`` (None: ``batch_size``) rows
    are labelled, ``y`` fp32 ``[B_l, F]`` the labelled rows' integer factor values (``index_factors``: derived from the
    image index); ``pre_process(x, y)`` when given.  The label columns are the table's ``latent_indices``, or the subset
    ``factors`` of them; ``.factor_sizes`` holds their sizes, for the solver's constructor.

    The unlabelled rows come from one ``torch.randperm`` per epoch, as ``DeviceLoader`` draws them (``len()`` and the batch
    sizes are its too).  The labelled subset of ``num_labelled`` image indices is drawn ONCE, before the first epoch, and
    never changes (``.labelled_indices``); every batch draws ``B_l`` of them uniformly with replacement.  All draws come
    from a private device generator seeded with ``seed`` -- the same seed repeats the same epochs, torch's global RNG
    streams are untouched.  One buffer, two gathers, no host round trip; the table's index flag is checked once, at the
    end of the epoch."""

    def __init__(self, table, batch_size, labelled_batch_size=None, num_labelled=1000, factors=None, seed=0,
                 drop_last=True, pre_process=None):
        if not isinstance(table, DeviceImageTable) or table.factor_sizes is None or table.latent_indices is None:
            raise ValueError("DeviceLabelledLoader: the table carries no factor_sizes / latent_indices")
        total = int(np.prod(table.factor_sizes, dtype=np.int64))
        if total != table.num_images:
            raise ValueError(f"DeviceLabelledLoader: the factors index {total} images, the table holds {table.num_images}")
        Bl = batch_size if labelled_batch_size is None else labelled_batch_size
        if batch_size < 1 or Bl < 1:
            raise ValueError("batch_size and labelled_batch_size must be positive")
        if not 1 <= num_labelled <= table.num_images:
            raise ValueError(f"num_labelled must lie in 1 .. {table.num_images}, the table's images (got {num_labelled})")
        lat = [int(i) for i in table.latent_indices]
        cols = lat if factors is None else [int(i) for i in factors]
        if not cols or len(set(cols)) != len(cols) or not set(cols) <= set(lat):
            raise ValueError(f"factors must name distinct latent factors out of {lat} (got {factors!r})")
        self.table, self.batch_size, self.labelled_batch_size = table, int(batch_size), int(Bl)
        self.num_labelled, self.columns, self.seed = int(num_labelled), tuple(cols), int(seed)
        self.drop_last, self.func = bool(drop_last), pre_process
        self.factor_sizes = tuple(int(table.factor_sizes[c]) for c in cols)
        self.labelled_indices = None
        self._gen = None

    def __len__(self):
        return len(DeviceLoader.batch_sizes(self.table.num_images, self.batch_size, self.drop_last))

    def __iter__(self):
        t, Bl = self.table, self.labelled_batch_size
        if self._gen is None:
            self._gen = torch.Generator(device=t.device).manual_seed(self.seed)
            self.labelled_indices = torch.randperm(t.num_images, generator=self._gen, device=t.device)[:self.num_labelled]
        order = torch.randperm(t.num_images, generator=self._gen, device=t.device)
        row = 0
        for n in DeviceLoader.batch_sizes(t.num_images, self.batch_size, self.drop_last):
            idx = order[row:row + n]
            row += n
            pick = torch.randint(self.num_labelled, (Bl,), generator=self._gen, device=t.device)
            lab = self.labelled_indices.index_select(0, pick)
            x = torch.empty((n + Bl,) + t.image_shape, dtype=torch.float32, device=t.device)
            t.gather(idx, out=x[:n], check=False)
            t.gather(lab, out=x[n:], check=False)
            y = index_factors(lab, t.factor_sizes, self.columns).to(torch.float32)
            yield self.func(x, y) if self.func is not None else (x, y)
        t.check()
