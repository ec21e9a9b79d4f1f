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
  * ``DeviceLoader`` feeds training from the table: one gather (+ flips) and one label ``index_select`` per batch.

Everything is opt-in (``VAESolver.use_device_dataset``); nothing here is used unless asked for.  Datasets that resize
(``resize != H``: PIL's bicubic filter) or decode files (UkiyoE) stay on the host path.
"""
import numpy as np
import torch

from . import abi
from .disentangle import FactorSampler

__all__ = ["DeviceImageTable", "DeviceFactorSampler", "DeviceLoader"]

UPLOAD_CHUNK_BYTES = 256 << 20


def _device(device):
    return torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())


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
    def from_dataset(cls, ds, device=None):
        """The table of a reference factor dataset (dataset.py:40-201): ``ds.imgs`` exactly as the class stored it -- the
        ``* 255`` of its constructor included, which wraps modulo 256 on uint8 -- and ``ds.latents_values`` as labels.
        Refuses, before touching the device, what ``__getitem__`` would not turn into ``imgs[i] / 255``: images that are
        not uint8 (``TypeError``) and a ``resize`` other than the stored height (``NotImplementedError``: the bicubic
        resize stays on the host path)."""
        imgs = np.asarray(ds.imgs)
        if imgs.dtype != np.uint8:
            raise TypeError(f"from_dataset: {type(ds).__name__}.imgs is {imgs.dtype}, not uint8")
        imgs = cls._check_arrays(imgs)
        resize = getattr(ds, "resize", None)
        if resize is not None and int(resize) != imgs.shape[1]:
            raise NotImplementedError(f"from_dataset: resize={resize} differs from the stored height {imgs.shape[1]}; "
                                      "resized datasets stay on the host path")
        table = cls.from_arrays(imgs, getattr(ds, "latents_values", None), device)
        try:        # the base class's properties raise NotImplementedError; a plain image dataset has neither
            table.factor_sizes, table.latent_indices = list(ds.factor_sizes), list(ds.latent_indices)
        except (AttributeError, NotImplementedError):
            table.factor_sizes = table.latent_indices = None
        return table

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
        C, H, W = self.image_shape
        abi.call("itcv_gather_u8", abi.ptr(self.images), self.num_images, C * H, W, abi.ptr(idx), n, abi.ptr(flip),
                 abi.ptr(out), self._flags.data_ptr(), abi.stream())
        if check and not from_host:
            self.check()
        return out

    def check(self):
        """Read the out-of-range flag of the gathers since the last check (one synchronisation); raises ``IndexError``."""
        if self._flags is not None and self._flags.item():
            self._flags.zero_()
            raise IndexError(f"a device index was outside [0, {self.num_images}); its image was returned as zeros")

    def labels(self, idx):
        """Rows ``idx`` of the label table (torch ``index_select``)."""
        if self.label_table is None:
            raise ValueError("this table has no labels")
        return self.label_table.index_select(0, self._index(idx)[0])


class DeviceFactorSampler(FactorSampler):
    """``FactorSampler`` whose observations come from a ``DeviceImageTable``: ``indices_from_factors`` (numpy, the same
    ``RandomState`` draws in the same order), one small host-to-device index copy, one gather.  With equal seeds it
    returns exactly ``FactorSampler``'s factors and observations.  ``dataset_or_table``: a dataset (its table is built
    with ``from_dataset`` unless ``table`` is given) or a table that carries ``factor_sizes`` / ``latent_indices``."""

    def __init__(self, dataset_or_table, device, seed=None, table=None):
        if isinstance(dataset_or_table, DeviceImageTable):
            table = dataset_or_table
            if table.factor_sizes is None:
                raise ValueError("DeviceFactorSampler: the table carries no factor_sizes / latent_indices")
        elif table is None:
            table = DeviceImageTable.from_dataset(dataset_or_table, device)
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
