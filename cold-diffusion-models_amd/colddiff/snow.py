"""The `diffusion` package of snowification/ on the fused snow kernels (csrc/k_snow.hip).

  diffusion/forward_process_impl.py:220-372   Snow
  diffusion/diffusion.py:177-193              the forward_process_type='Snow' branch of GaussianDiffusion
Everything else of the package is file for file the decolorization package's and is shared with it (colddiff/decolor.py): `SnowDiffusion`
is `DecolorDiffusion` with its two hooks overridden -- which forward process is built, and how "the state of every row after its step
count" is computed.

`Snow.forward(x, i, og=)` never reads `x`: the state after any number of steps is a pointwise function of the original image and the last
step's index.  So `q_sample`, a reverse step of either sampling routine and the forward leg of `sample()` are ONE `cdf_snow_chain` launch
each, where the reference runs up to T passes of about ten elementwise launches, a `torch.stack` and a gather per row.

The host keeps what has to stay the reference's: the numpy draws (state saved, seeded with 123321 and restored unless `random_snow`), the
base layer through `scipy.ndimage.zoom(order=1)` in float64, the one `np.random.uniform()` and the per-step `torch.randperm` of
`single_snow`.  The threshold makes the base discontinuous -- a zoom value one ulp off flips a pixel across it -- so neither the normal
generator nor the zoom moves to the device; threshold, clip and motion blur of all T steps are one `cdf_snow_layers` launch.
"""
import numpy as np
import torch

from . import degrade as D
from . import runtime as rt
from .decolor import _FINAL_ROUTINES, DecolorDiffusion, DeColorization, ForwardProcessBase
from .runtime import P

# per snow_level: (mean, std of the base, zoom factor, taps of the motion blur), then start / end of the threshold, blur sigma and
# brightness schedules (forward_process_impl.py:261-292)
_LEVELS = {
    1: ((0.1, 0.3, 3, 5), (0.7, 0.3), (0.5, 5.0), (0.95, 0.7)),
    2: ((0.55, 0.3, 2.5, 11), (1.15, 0.7), (0.05, 12), (0.95, 0.55)),
    3: ((0.55, 0.3, 2.5, 11), (1.15, 0.7), (0.05, 16), (0.95, 0.4)),
    4: ((0.55, 0.3, 2.5, 11), (1.15, 0.55), (0.05, 20), (0.95, 0.3)),
}


def _zoom():
    try:
        from scipy.ndimage import zoom
    except ImportError as e:
        raise ImportError("forward_process_type='Snow' needs scipy (the snow base layer is scipy.ndimage.zoom(order=1) of a normal field, "
                          "as upstream builds it), which is not installed") from e
    return zoom


def clipped_zoom(img, zoom_factor):
    """The centre of a square [side,side,1] array magnified by zoom_factor (bilinear, scipy) and cut back to side x side
    (forward_process_impl.py:32-42; float64 in, float64 out)."""
    side = img.shape[0]
    crop = int(np.ceil(side / zoom_factor))
    lo = (side - crop) // 2
    grown = _zoom()(img[lo:lo + crop, lo:lo + crop], (zoom_factor, zoom_factor, 1), order=1)
    off = (grown.shape[0] - side) // 2
    return grown[off:off + side, off:off + side]


def snow_layers(base, thres, taps, vertical):
    """One `cdf_snow_layers` launch: base [L,H,W], thres [T], taps [T,k], vertical [T,L] (uint8) -> planes [T,L,H,W]."""
    L, H, W = base.shape
    T, k = taps.shape
    out = torch.empty((T, L, H, W), device=base.device, dtype=torch.float32)
    rt.lib().cdf_snow_layers(P(base), P(thres), P(taps), P(vertical), P(out), H, W, L, T, k, rt.stream(base))
    return out


class Snow(ForwardProcessBase):
    """Constructor arguments and attribute names of the reference class.  `snow` / `snow_rot` are lists of [L,3,H,W] views of ONE
    [T,L,H,W] plane storage (the reference's three channels are identical), built by `cdf_snow_layers` on the device of first use and
    again after a `reset_parameters` that regenerates."""

    def __init__(self, image_size=(32, 32), snow_level=1, num_timesteps=50, snow_base_path=None, random_snow=False, single_snow=False,
                 batch_size=32, load_snow_base=False, fix_brightness=False):
        self.num_timesteps = num_timesteps
        self.random_snow = random_snow
        self.snow_level = snow_level
        self.image_size = image_size
        self.single_snow = single_snow
        self.batch_size = batch_size
        self._device = None
        self.generate_snow_layer()
        self.fix_brightness = fix_brightness

    @torch.no_grad()
    def reset_parameters(self, batch_size=-1):
        if batch_size != -1:
            self.batch_size = batch_size
        if self.random_snow:
            self.generate_snow_layer()

    @torch.no_grad()
    def generate_snow_layer(self):
        """The host part, draw for draw in the reference's order; the planes themselves are built on the device when first read."""
        if not self.random_snow:
            rstate = np.random.get_state()
            np.random.seed(123321)
        (loc, scale, zoom_factor, k), thres, sigma, br = _LEVELS[self.snow_level]
        T = self.num_timesteps
        self.snow_thres_list = torch.linspace(thres[0], thres[1], T).tolist()
        self.mb_sigma_list = torch.linspace(sigma[0], sigma[1], T).tolist()
        self.br_coef_list = torch.linspace(br[0], br[1], T).tolist()
        size = tuple(self.image_size) if isinstance(self.image_size, (tuple, list)) else (self.image_size, self.image_size)
        layers = []
        for _ in range(self.batch_size if self.single_snow else 1):
            cs = np.random.normal(size=size, loc=loc, scale=scale)
            layers.append(clipped_zoom(cs[..., np.newaxis], zoom_factor))
        base = np.concatenate(layers, axis=2)                                   # [H,W,L] float64
        vertical_snow = bool(np.random.uniform() > 0.5)
        L = base.shape[2]
        vertical = torch.full((T, L), 1 if vertical_snow else 0, dtype=torch.uint8)
        if self.single_snow:
            for i in range(T):
                vidx = torch.randperm(L)[:int(L / 2)]
                vertical[i] = 0
                vertical[i, vidx] = 1
        if not self.random_snow:
            np.random.set_state(rstate)
        self.snow_base = torch.Tensor(base).permute(2, 0, 1).contiguous()      # [L,H,W] fp32, as torch.Tensor() casts it upstream
        self.vertical = vertical
        self.taps = torch.stack([D.gaussian_1d(k, s) for s in self.mb_sigma_list])
        # float32(br) and float32(1.0 - br): the tensor arithmetic upstream rounds the two python doubles separately
        self._host = (torch.tensor(self.snow_thres_list, dtype=torch.float32), torch.tensor(self.br_coef_list, dtype=torch.float32),
                      torch.tensor([1.0 - b for b in self.br_coef_list], dtype=torch.float32))
        self._planes = None
        self._tables = None

    # -- device storage ---------------------------------------------------------------------------------
    def planes(self, device=None):
        """[T,L,H,W] on `device` (default: where they were last used, else the HIP device)."""
        if device is None:
            device = self._device if self._device is not None else torch.device('cuda' if rt._lib_override is None else 'cpu')
        device = torch.device(device)
        if device.type == 'cuda' and device.index is None:
            device = torch.device('cuda', torch.cuda.current_device())
        if self._planes is None or self._planes.device != device:
            thres, br, omb = (v.to(device) for v in self._host)
            self._planes = snow_layers(rt.check(self.snow_base.to(device)), thres, self.taps.to(device), self.vertical.to(device))
            self._tables = (br, omb)
            self._device = device
        return self._planes

    def set_planes(self, planes):
        """Replace the plane storage ([T,L,H,W]; e.g. planes another implementation made) until the next regeneration."""
        planes = planes.contiguous().float()
        _, br, omb = (v.to(planes.device) for v in self._host)
        self._planes, self._tables, self._device = planes, (br, omb), planes.device

    @property
    def snow(self):
        p = self.planes()
        return [p[i][:, None].expand(-1, 3, -1, -1) for i in range(p.shape[0])]

    @property
    def snow_rot(self):
        p = self.planes().flip(dims=[2, 3])
        return [p[i][:, None].expand(-1, 3, -1, -1) for i in range(p.shape[0])]

    # -- the process ------------------------------------------------------------------------------------
    def chain(self, og, start=None, nsteps=0, nsteps_b=None, nmax=0, want_total=False, want_snap=False, img=None, layer_b=None):
        """One `cdf_snow_chain` launch on [B,3,H,W]: row b has the count nsteps_b[b] (int64 tensor) or `nsteps`; its state after n steps is
        D(og_b, n - 1), `start_b` (default og_b) for n = 0, and for a negative count the row of og.  -> y [, total (state after nmax steps)]
        [, snap (state after min(n_b, nmax - 1) steps)]; with img the Algorithm-2 combine (img - y) + snap takes y's place."""
        og = D._img(og)
        B, C, H, W = og.shape
        planes = self.planes(og.device)
        T, L = planes.shape[0], planes.shape[1]
        if C != 3 or (H, W) != tuple(planes.shape[2:]):
            raise RuntimeError(f"Snow: images of shape {tuple(og.shape)} against snow planes of {tuple(planes.shape[2:])} (3 channels)")
        if L > 1 and layer_b is None and B != L:
            raise RuntimeError(f"single_snow pairs row k of the forwarded batch with snow layer k: {B} rows against {L} layers "
                               f"(upstream fails here with a broadcast error)")
        nb = D._steps(nsteps_b, B)
        if nb is not None and nb.device != og.device:
            nb = nb.to(og.device)
        lb = None if layer_b is None else D._steps(layer_b, B).to(og.device)
        start = None if start is None else D._img(start)
        img = None if img is None else D._img(img)
        y = torch.empty_like(og)
        total = torch.empty_like(og) if want_total else None
        snap = torch.empty_like(og) if want_snap else None
        br, omb = self._tables
        rt.lib().cdf_snow_chain(P(og), P(start), P(y), P(total), P(snap), P(img), P(planes), P(br), P(omb), P(nb), P(lb), B, H * W, L, T,
                                int(nsteps), int(nmax), 1 if self.fix_brightness else 0, rt.stream(og))
        out = (y,) + ((total,) if want_total else ()) + ((snap,) if want_snap else ())
        return out[0] if len(out) == 1 else out

    @torch.no_grad()
    def total_forward(self, x_in):
        return self.forward(None, self.num_timesteps - 1, og=x_in)

    @torch.no_grad()
    def forward(self, x, i, og=None):
        og = rt.check(og)
        i = int(i)
        if i < 0:
            i += self.num_timesteps                                             # (upstream indexes python lists)
        return self.chain(og, nsteps=i + 1)


class SnowDiffusion(DecolorDiffusion):
    """`GaussianDiffusion` of the snowification package: both forward process types, the body of `DecolorDiffusion`."""

    def _build_forward_process(self, forward_process_type, *, load_snow_base=False, load_path=None, fix_brightness=False, results_folder=None,
                               **decolor_kw):
        if forward_process_type != 'Snow':
            if forward_process_type == 'Decolorization':
                return DeColorization(channels=self.channels, num_timesteps=self.num_timesteps, to_lab=self.to_lab, **decolor_kw)
            raise NotImplementedError(f"forward_process_type={forward_process_type!r}: 'Snow' and 'Decolorization' are the forward "
                                      f"processes of this package")
        import os
        # upstream computes this path and never reads or writes it (nor does Snow look at load_snow_base)
        if load_path is not None:
            snow_base_path, load_snow_base = load_path.replace('model.pt', 'snow_base.npy'), True
        else:
            snow_base_path, load_snow_base = (None if results_folder is None else os.path.join(results_folder, 'snow_base.npy')), False
        return Snow(image_size=self.image_size, snow_level=self.snow_level, random_snow=self.random_snow, num_timesteps=self.num_timesteps,
                    snow_base_path=snow_base_path, batch_size=self.batch_size, single_snow=self.single_snow, load_snow_base=load_snow_base,
                    fix_brightness=fix_brightness)

    def _is_snow(self):
        return isinstance(self.forward_process, Snow)

    def _chain(self, og, start=None, **kw):
        if not self._is_snow():
            return super()._chain(og, start=start, **kw)
        return self.forward_process.chain(og, start=start, **kw)

    def _paired(self):
        return self._is_snow() and self.forward_process.single_snow

    def q_sample(self, x_start, t, return_total_blur=False):
        if self._paired():
            # upstream forwards the rows with t != -1 only: fewer rows than layers is its broadcast error (one host read, this option only)
            kept = int((D._steps(t, x_start.shape[0]) != -1).sum())
            if 0 < kept < x_start.shape[0]:
                raise RuntimeError(f"single_snow pairs row k of the forwarded batch with snow layer k: q_sample forwards {kept} of "
                                   f"{x_start.shape[0]} rows (t == -1 rows are left out; upstream fails here with a broadcast error)")
        return super().q_sample(x_start, t, return_total_blur=return_total_blur)

    @torch.no_grad()
    def sample_one_step(self, img, t, init_pred=None, _tmax=None):
        if self._paired() and _tmax is None and self.train_routine in _FINAL_ROUTINES and self.sampling_routine in ('default', 'x0_step_down'):
            # rows leave upstream's loop at their own t: unequal step counts forward fewer rows than layers (the samplers pass equal t)
            n = D._steps(t, img.shape[0])
            n = (n - 1).clamp(min=0) if self.sampling_routine == 'default' else n
            if int(n.min()) != int(n.max()):
                raise RuntimeError("single_snow pairs row k of the forwarded batch with snow layer k: sample_one_step with unequal t "
                                   "forwards a subset of the rows (upstream fails here with a broadcast error)")
        return super().sample_one_step(img, t, init_pred=init_pred, _tmax=_tmax)

    def prepare(self, x, x2=None, t=None):
        assert self.fusable()
        if t is None:
            t = self._draw_t(x)
        self.forward_process.reset_parameters()                                  # (p_losses' first line: with random_snow new planes)
        return x, t, self._q_sample_nonneg(x, t)
