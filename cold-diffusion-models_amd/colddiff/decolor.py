"""The `diffusion` package of decolor-diffusion/ (the paper's colourization experiment) on the fused colour kernels.

Constructor arguments, attribute names, method names, return values and `state_dict` layout follow
  diffusion/forward_process_impl.py:131-218   DeColorization
  diffusion/diffusion.py:110-490              GaussianDiffusion
  diffusion/diffusion.py:563-760              Trainer
  diffusion/model/unet_convnext.py:125-226    UnetConvNextBlock
  diffusion/utils.py:113-222                  rgb2lab / lab2rgb
What differs is the execution.  The reference runs the forward process as up to T `nn.Conv2d(3, 3, 1)` launches plus a `torch.stack` of
every intermediate batch and a python gather per row; here `q_sample` is ONE `cdf_color_chain` launch whatever `t.max()` is (the pixel's
three channels stay in registers for the whole chain) and a reverse step of either sampling routine is one more.  The index arithmetic of
`q_sample` (the `t == -1` rows of the Step routines, quirk included) is resolved into the per-row step vector before the launch.
"""
from pathlib import Path

import torch
from torch import nn

from . import degrade as D
from . import metrics, parallel
from . import runtime as rt
from .data import RANDOM_AUG, CacheUnfit, DeviceImageCache, DeviceLoader, cycle, make_grid, save_image, write_grid
from .diffusion import TwoPhase, _full_step
from .evaluate import rep3, sweep_ranks
from .runtime import P
from .trainer import Recipe, Trainer
from .unet import Unet, exists


# ===================================================================================================
# kernel calls
# ===================================================================================================
def color_chain(x, table, nsteps=0, nsteps_b=None, nmax=0, want_total=False, want_snap=False, img=None, lab=False):
    """One launch of the colour chain on [B,3,H,W]: row b runs nsteps_b[b] (int64 tensor; negative = row passed through) or `nsteps`
    steps of `table` ([T,3,3]).  -> y [, total (state after nmax steps)] [, snap (state after min(n_b, nmax - 1) steps)]; with img the
    Algorithm-2 combine (img - x_n) + snap takes y's place."""
    x = D._img(x)
    B, C, H, W = x.shape
    nb = D._steps(nsteps_b, B)
    if nb is not None and nb.device != x.device:
        nb = nb.to(x.device)            # (a step vector on the host would hand the kernel a host pointer)
    y = torch.empty_like(x)
    total = torch.empty_like(x) if want_total else None
    snap = torch.empty_like(x) if (want_snap or img is not None) else None
    img = None if img is None else D._img(img)
    if table.device != x.device:
        table = table.to(x.device)
    rt.lib().cdf_color_chain(P(x), P(y), P(total), P(snap), P(img), P(table), P(nb), B, C, H * W, table.shape[0], int(nsteps), int(nmax),
                             1 if lab else 0, rt.stream(x))
    out = (y,) + ((total,) if want_total else ()) + ((snap,) if want_snap else ())
    return out[0] if len(out) == 1 else out


def _lab_convert(image, to_rgb):
    if image.dim() < 3 or image.shape[-3] != 3:
        raise ValueError(f"Input size must have a shape of (*, 3, H, W). Got {image.shape}")
    x = D._img(image)
    shape = x.shape
    x4 = x.reshape(-1, 3, shape[-2], shape[-1])
    y = torch.empty_like(x4)
    rt.lib().cdf_lab_convert(P(x4), P(y), x4.shape[0], 3, shape[-2] * shape[-1], to_rgb, rt.stream(x4))
    return y.reshape(shape)


def rgb2lab(image_old):
    """RGB in (-1, 1) -> Lab (L 0..100), D65 / observer 2 (utils.py:113-163)."""
    return _lab_convert(image_old, 0)


def lab2rgb(image, clip=True):
    """Lab -> RGB in [-1, 1] (utils.py:166-222); the kernel always clips, as every caller upstream does."""
    if not clip:
        raise NotImplementedError("lab2rgb(clip=False): the kernel clamps to [0, 1] like every call of the package")
    return _lab_convert(image, 1)


def _axpby(a, b, beta):
    """a + beta * b on images (`cdf_axpby`; beta = +-1: the exact fp32 sum / difference)."""
    a, b = D._img(a), D._img(b)
    out = a.clone()
    W = out.shape[-1]
    rt.lib().cdf_axpby(P(out), W, P(b), W, out.numel() // W, W, 1.0, float(beta), rt.stream(out))
    return out


class MeanShift(torch.autograd.Function):
    """out = (y - mean_b(x)) + mean_b(y), per-image means over C*H*W (unet_convnext.py:198, 222-224); gradient to y only."""

    @staticmethod
    def forward(ctx, x, y):
        x, y = D._img(x), D._img(y)
        B, n = y.shape[0], y[0].numel()
        L = rt.lib()
        ws = torch.empty((B * L.cdf_mean_shift_nchunk(n) * 2,), device=y.device, dtype=torch.float32)
        out = torch.empty_like(y)
        L.cdf_mean_shift(P(x), P(y), P(out), P(ws), B, n, rt.stream(y))
        return out

    @staticmethod
    def backward(ctx, dy):
        dy = dy.contiguous().float()
        B, n = dy.shape[0], dy[0].numel()
        L = rt.lib()
        ws = torch.empty((B * L.cdf_mean_shift_nchunk(n) * 2,), device=dy.device, dtype=torch.float32)
        dx = torch.empty_like(dy)
        L.cdf_mean_shift_bwd(P(dy), P(dx), P(ws), B, n, rt.stream(dy))
        return None, dx


# ===================================================================================================
# the forward process
# ===================================================================================================
class ForwardProcessBase:
    def forward(self, x, i):
        pass

    @torch.no_grad()
    def reset_parameters(self, batch_size=32):
        pass


class DeColorization(ForwardProcessBase):
    """Per step a 3 x 3 colour mix  ema * I + (1 - ema) * ones / C  (the weight of the reference's 1 x 1 conv, built on the host with the
    same torch expressions: bit-equal); `kernels` keeps the list of [C,C,1,1] weights, `table` the same as one [T,C,C] tensor the kernel
    reads."""

    def __init__(self, decolor_routine='Constant', decolor_ema_factor=0.9, decolor_total_remove=False, num_timesteps=50, channels=3,
                 to_lab=False):
        self.decolor_routine = decolor_routine
        self.decolor_ema_factor = decolor_ema_factor
        self.decolor_total_remove = decolor_total_remove
        self.channels = channels
        self.num_timesteps = num_timesteps
        self.device_of_kernel = 'cuda'
        self.kernels = self.get_kernels()
        self.to_lab = to_lab
        self.table = torch.stack([k[:, :, 0, 0] for k in self.kernels]).contiguous() if self.kernels else torch.zeros(0, channels, channels)
        ones = torch.ones((self.channels, self.channels)) / float(self.channels)
        self.total_table = ones[None].contiguous()

    def get_conv(self, decolor_ema_factor):
        """The weight [C,C,1,1] of the reference's conv for this factor (a tensor, not a module: the kernel applies it)."""
        ori_color_weight = torch.eye(self.channels)[:, :, None, None]
        decolor_weight = torch.ones((self.channels, self.channels)) / float(self.channels)
        decolor_weight = decolor_weight[:, :, None, None]
        return decolor_ema_factor * ori_color_weight + (1.0 - decolor_ema_factor) * decolor_weight

    def get_kernels(self):
        kernels = []
        last = self.num_timesteps - 1
        if self.decolor_routine == 'Constant':
            for i in range(self.num_timesteps):
                kernels.append(self.get_conv(0.0 if (i == last and self.decolor_total_remove) else self.decolor_ema_factor))
        elif self.decolor_routine == 'Linear':
            diff = 1.0 / self.num_timesteps
            start = 1.0
            for i in range(self.num_timesteps):
                if i == last and self.decolor_total_remove:
                    kernels.append(self.get_conv(0.0))
                else:
                    ema_factor = 1 - diff / start            # (each step removes the same absolute share of colour)
                    start = start * ema_factor
                    kernels.append(self.get_conv(ema_factor))
        return kernels

    def _table(self, device):
        if self.table.device != device:
            self.table = self.table.to(device)
            self.total_table = self.total_table.to(device)
        return self.table

    def forward(self, x, i, og=None):
        """Step i alone (the sampler and q_sample run whole chains through `color_chain`)."""
        x = rt.check(x)
        if x.shape[0] == 0:
            return x.clone()
        table = self._table(x.device)
        return color_chain(x, table[int(i):int(i) + 1], nsteps=1, lab=self.to_lab)

    def total_forward(self, x_in):
        x_in = rt.check(x_in)
        self._table(x_in.device)
        return color_chain(x_in, self.total_table, nsteps=1, lab=self.to_lab)


# ===================================================================================================
# GaussianDiffusion
# ===================================================================================================
_FINAL_ROUTINES = ('Final', 'Final_random_mean', 'Final_small_noise', 'Final_random_mean_and_actual')


class DecolorDiffusion(TwoPhase, nn.Module):
    def __init__(self, denoise_fn, *, image_size, device_of_kernel, one_shot_denoise_fn=None, channels=3, timesteps=1000, loss_type='l1',
                 kernel_std=0.1, kernel_size=3, forward_process_type='Decolorization', train_routine='Final', sampling_routine='default',
                 start_kernel_std=0.01, target_kernel_std=1.0, decolor_routine='Constant', decolor_ema_factor=0.9,
                 decolor_total_remove=True, snow_level=1, random_snow=False, to_lab=False, order_seed=-1.0, recon_noise_std=0.0,
                 load_snow_base=False, load_path=None, batch_size=32, single_snow=False, fix_brightness=False, results_folder=None):
        super().__init__()
        self.channels = channels
        self.image_size = image_size
        self.denoise_fn = denoise_fn
        self.device_of_kernel = device_of_kernel
        self.num_timesteps = int(timesteps)
        self.loss_type = loss_type
        self.train_routine = train_routine
        self.sampling_routine = sampling_routine
        self.snow_level = snow_level
        self.random_snow = random_snow
        self.batch_size = batch_size
        self.single_snow = single_snow
        self.to_lab = to_lab
        self.recon_noise_std = recon_noise_std
        self.forward_process = self._build_forward_process(
            forward_process_type, decolor_routine=decolor_routine, decolor_ema_factor=decolor_ema_factor,
            decolor_total_remove=decolor_total_remove, load_snow_base=load_snow_base, load_path=load_path, fix_brightness=fix_brightness,
            results_folder=results_folder)

    # -- the two hooks a package with another forward process overrides (colddiff/snow.py) ---------------
    def _build_forward_process(self, forward_process_type, *, decolor_routine, decolor_ema_factor, decolor_total_remove, **snow_kw):
        if forward_process_type == 'Decolorization':
            return DeColorization(decolor_routine=decolor_routine, decolor_ema_factor=decolor_ema_factor,
                                  decolor_total_remove=decolor_total_remove, channels=self.channels,
                                  num_timesteps=self.num_timesteps, to_lab=self.to_lab)
        elif forward_process_type == 'Snow':
            raise NotImplementedError("forward_process_type='Snow' is not built (the snowification forward process needs host-side snow "
                                      "layers; this package implements forward_process_type='Decolorization')")
        else:
            raise NotImplementedError(f"forward_process_type={forward_process_type!r}: 'Decolorization' is the forward process of this package")

    def _chain(self, og, start=None, **kw):
        """The state of every row after its step count, in ONE launch (`color_chain`'s keywords).  `og`: the images the process degrades;
        `start`: what a row that takes zero steps holds, when that is not `og` (the noised prediction of `x0_step_down`) -- the colour
        chain, a composition of steps, simply starts there."""
        x = D._img(og if start is None else start)
        return color_chain(x, self._table(x.device), lab=self.to_lab, **kw)

    # -- helpers --------------------------------------------------------------------------------------
    def _hw(self):
        s = self.image_size
        if type(s) is tuple:
            img_w, img_h = s
        else:
            img_h, img_w = s, s
        return img_h, img_w

    def _draw_t(self, x):
        b, c, h, w = x.shape
        img_h, img_w = self._hw()
        assert h == img_h and w == img_w, f'height and width of image must be {self.image_size}'
        return torch.randint(0, self.num_timesteps, (b,), device=x.device).long()

    def _table(self, device):
        return self.forward_process._table(device)

    def _q_sample_nonneg(self, x_start, t):
        """q_sample for t >= 0 everywhere (what forward() draws): n_b = t_b + 1 computed on the device, nothing synchronises."""
        x_start = rt.check(x_start)
        return self._chain(x_start, nsteps_b=t + 1)

    # -- sampling -------------------------------------------------------------------------------------
    # sampler graph mode (colddiff/graphsample.py) is declined by this package and by the snowification package built on it
    _SG_WHY = "the colour / snow reverse step takes host values per step (t.max(), the per-call forward-process state): not captured"
    # `sample` and `all_sample` keep loops of their own: their step is the public `sample_one_step`, which calls the network itself and
    # takes the step vector, where the shared walk (SampleGraphMixin._walk, used by forward_and_backward) calls the network and asks the
    # core for the update only

    @torch.no_grad()
    def sample_one_step(self, img, t, init_pred=None, _tmax=None):
        """One reverse step (diffusion.py:196-245).  `_tmax`: t.max() when the caller knows it (the samplers do: every row has the same
        t), otherwise read from the device as upstream's `range(t.max())` does."""
        img = rt.check(img)
        t = t.to(img.device)                                   # (a step vector on the host would reach the kernels as a host pointer)
        x = self.prediction_step_t(img, t, init_pred)
        direct_recons = x.clone()
        if self.recon_noise_std > 0.0:
            self.recon_noise_std_array = torch.linspace(0.0, self.recon_noise_std, steps=self.num_timesteps)
        if self.train_routine in _FINAL_ROUTINES:
            t = D._steps(t, img.shape[0])
            if self.sampling_routine == 'default':
                # rows advance while cur_time < t - 1, for i in range(t.max() - 1): n_b = max(t_b - 1, 0) steps
                x = self._chain(x, nsteps_b=(t - 1).clamp(min=0))
            elif self.sampling_routine == 'x0_step_down':
                x_times = None
                if self.recon_noise_std > 0.0:
                    x_times = x + torch.normal(0.0, self.recon_noise_std, size=x.size(), device=x.device)
                # x_times: t_b steps; x_times_sub_1 is re-cloned from the WHOLE batch at the top of every global iteration, so a row holds
                # its state after min(t_b, t.max() - 1) steps (and x_times itself when t.max() == 0): the kernel's `snap`
                tmax = int(t.max()) if _tmax is None else int(_tmax)          # (upstream's `range(t.max())`; the samplers pass it)
                x = self._chain(x, start=x_times, nsteps_b=t, nmax=tmax, img=img)
        elif self.train_routine == 'Step':
            img = x
        elif self.train_routine == 'Step_Gradient':
            x = _axpby(img, x, 1.0)
        return x, direct_recons

    @torch.no_grad()
    def sample_multi_step(self, img, t_start, t_end):
        """Rows walk from t_start[b] down to t_end[b], one `direct_recons` per pass over the rows still above their end (diffusion.py:247-256)."""
        out = img.clone()
        while True:
            rows = torch.where(t_start > t_end)[0]
            if len(rows) == 0:
                return out
            out[rows] = self.sample_one_step(out[rows], t_start[rows])[1]
            t_start = t_start - 1

    @torch.no_grad()
    def sample(self, batch_size=16, img=None, t=None, graph=None):
        self._sg_eager(graph, self._SG_WHY)
        self.forward_process.reset_parameters(batch_size=batch_size)
        if t == None:                                          # noqa: E711 (as upstream)
            t = self.num_timesteps
        img = rt.check(img)
        # the t forward steps of diffusion.py:270-273 as one launch
        img = self._chain(img, nsteps=t) if t > 0 else img.clone()
        init_pred = None
        xt = img
        direct_recons = None
        while t:
            step = _full_step(batch_size, t - 1, img.device)
            x, cur_direct_recons = self.sample_one_step(img, step, init_pred=init_pred, _tmax=t - 1)
            if direct_recons is None:
                direct_recons = cur_direct_recons
            img = x
            t = t - 1
        if self.to_lab:
            xt = lab2rgb(xt)
            direct_recons = lab2rgb(direct_recons)
            img = lab2rgb(img)
        return {'xt': xt, 'direct_recons': direct_recons, 'recon': img}

    @torch.no_grad()
    def all_sample(self, batch_size=16, img=None, t=None, times=None, res_dict=None, ends_only=False, graph=None):
        """diffusion.py:292-342.  `ends_only=True` (this engine's addition): -> (X_ts[0], X_0s[0], X_0s[-1]) of the full call, bit for
        bit, as device tensors -- the three the metric sweep reads -- without the other 2 T - 3 `lab2rgb` launches and host copies."""
        self._sg_eager(graph, self._SG_WHY)
        self.forward_process.reset_parameters(batch_size=batch_size)
        if t == None:                                          # noqa: E711
            t = self.num_timesteps
        if times == None:                                      # noqa: E711
            times = t
        img_forward_list = []
        img = self.forward_process.total_forward(rt.check(img))
        X_0s, X_ts = [], []
        init_pred = None
        first = last = None
        while times:
            step = _full_step(img.shape[0], times - 1, img.device)
            img, direct_recons = self.sample_one_step(img, step, init_pred=init_pred, _tmax=times - 1)
            if ends_only:
                first = (img, direct_recons) if first is None else first
                last = direct_recons
            else:
                # (upstream converts after .cpu(); the conversion is a kernel, so it runs before the copy)
                X_0s.append((lab2rgb(direct_recons) if self.to_lab else direct_recons).cpu())
                X_ts.append((lab2rgb(img) if self.to_lab else img).cpu())
            times = times - 1
        if ends_only:
            if first is None:
                raise ValueError("all_sample(ends_only=True) needs at least one step")
            rgb = lab2rgb if self.to_lab else (lambda z: z)
            x0_first = rgb(first[1])
            return rgb(first[0]), x0_first, (x0_first if last is first[1] else rgb(last))
        init_pred_clone = None
        return X_0s, X_ts, init_pred_clone, img_forward_list

    # -- forward process ------------------------------------------------------------------------------
    def q_sample(self, x_start, t, return_total_blur=False):
        """diffusion.py:344-388 as one launch.  Upstream filters the rows with t != -1, runs the chain to max(t) on them, and then picks
        `all_blurs[t[step], step]` with `step` counting the FILTERED rows but `t` unfiltered: the k-th kept row takes the step count of
        row k of the batch (a -1 there indexes the last state).  That arithmetic is resolved here into one step count per row -- by a
        cumulative-sum index on the device, so that the call does not wait for the host -- and rows with t == -1 pass through."""
        x_start = rt.check(x_start)
        B = x_start.shape[0]
        t = D._steps(t, B).to(x_start.device)
        keep = t != -1
        pos = (torch.cumsum(keep, 0) - 1).clamp(min=0)          # a kept row's position among the kept rows
        picked = t[pos]                                          # ... and the step upstream reads for it: t at THAT index
        mx = t.max()
        nb = torch.where(keep, torch.where(picked < 0, mx, picked) + 1, torch.full_like(t, -1))
        if return_total_blur:
            # the total blur is the state after max(t) + 1 steps: ONE scalar read, as upstream's `range(max_iters + 1)`
            max_iters = int(mx)
            if max_iters < 0:
                return x_start.clone()                           # (every row is t == -1: upstream returns the single tensor)
            return self._chain(x_start, nsteps_b=nb, nmax=max_iters + 1, want_total=True)
        return self._chain(x_start, nsteps_b=nb)   # nothing synchronises; all rows -1: every row passes through

    def loss_func(self, pred, true):
        if self.loss_type == 'l1':
            return D.loss(pred, true, 'l1')
        elif self.loss_type == 'l2':
            return D.loss(pred, true, 'l2')
        elif self.loss_type == 'sqrt':
            return D.loss(pred, true, 'l1').sqrt()
        else:
            raise NotImplementedError()

    def prediction_step_t(self, img, t, init_pred=None):
        return self.denoise_fn(img, t)

    def loss_prepared(self, prep):
        x_start, t, x_deg = prep
        return self.loss_func(x_start, self.denoise_fn(x_deg, t))

    def prepare(self, x, x2=None, t=None):
        assert self.fusable()
        if t is None:
            t = self._draw_t(x)
        return x, t, self._q_sample_nonneg(x, t)

    def p_losses(self, x_start, t, t_pred=None):
        b, c, h, w = x_start.shape
        self.forward_process.reset_parameters()
        # (upstream asks q_sample for the total blur too and never reads it: not computed)
        if self.train_routine == 'Final':
            x_blur = self.q_sample(x_start=x_start, t=t)
            x_recon = self.denoise_fn(x_blur, t)
            loss = self.loss_func(x_start, x_recon)
        elif self.train_routine == 'Step_Gradient':
            x_blur = self.q_sample(x_start=x_start, t=t)
            x_blur_sub = self.q_sample(x_start=x_start, t=t - 1)
            x_blur_diff = _axpby(x_blur_sub, x_blur, -1.0)
            x_blur_diff_pred = self.denoise_fn(x_blur, t)
            loss = self.loss_func(x_blur_diff, x_blur_diff_pred)
        elif self.train_routine == 'Step':
            x_blur = self.q_sample(x_start=x_start, t=t)
            x_blur_sub = self.q_sample(x_start=x_start, t=t - 1)
            x_blur_sub_pred = self.denoise_fn(x_blur, t)
            loss = self.loss_func(x_blur_sub, x_blur_sub_pred)
        return loss

    def forward(self, x, *args, **kwargs):
        t = self._draw_t(x)
        # (upstream also draws a `t_pred` per row with b host round trips; p_losses never reads it: DESIGN.md section 7)
        if self.train_routine == 'Final' and not args and not kwargs:
            return self.loss_prepared(self.prepare(x, t=t))
        return self.p_losses(x, t, None, *args, **kwargs)

    @torch.no_grad()
    def forward_and_backward(self, batch_size=16, img=None, t=None, times=None, eval=True, graph=None):
        self._sg_eager(graph, self._SG_WHY)
        self.denoise_fn.eval()
        if t == None:                                          # noqa: E711
            t = self.num_timesteps
        img = rt.check(img)
        Forward = [img]
        for i in range(t):
            n_img = self._chain(img, nsteps=i + 1)       # q_sample(img, full(i))
            Forward.append(n_img)
        Backward = []
        # img - q_sample(x1_bar, t - 1) + q_sample(x1_bar, t - 2): t steps, the state one step earlier, and the combine, in one launch
        # (t - 1 == 0: xt_sub1_bar = x1_bar itself = the state after 0 steps)
        _, img = self._walk(n_img, t, batch_size, lambda x_t, x1_bar, t, tb: self._chain(x1_bar, nsteps=t, nmax=t, img=x_t),
                            collect=lambda x1_bar, x_t: Backward.append(x_t))
        return Forward, Backward, img


# ===================================================================================================
# the network
# ===================================================================================================
class UnetConvNextBlock(Unet):
    """`Unet` with the reference's parameter order, `forward(x, time=None)` and the mean-shifted output (unet_convnext.py:125-226): same
    sub-module names, `state_dict` keys and parameter creation order, so the same seed gives the same initial weights."""

    def __init__(self, dim, out_dim=None, dim_mults=(1, 2, 4, 8), channels=3, with_time_emb=True, output_mean_scale=False, residual=False):
        super().__init__(dim, out_dim=out_dim, dim_mults=dim_mults, channels=channels, with_time_emb=with_time_emb, residual=residual)
        self.output_mean_scale = output_mean_scale

    def forward(self, x, time=None):
        if time is None or not exists(self.time_mlp):
            assert not exists(self.time_mlp), 'time emb must be passed in'
            time = torch.zeros((x.shape[0],), dtype=torch.long, device=x.device)        # (never read: the network has no time MLP)
        out = super().forward(x, time)
        if self.output_mean_scale and not self.residual:
            out = MeanShift.apply(x, out)
        return out


def get_model(args, with_time_emb=True):
    """model/get_model.py: `--model UnetConvNext` is the 64-wide (1, 2, 4, 8) network."""
    if args.model == 'UnetConvNext':
        return UnetConvNextBlock(dim=64, dim_mults=(1, 2, 4, 8), channels=3, with_time_emb=with_time_emb, residual=False)
    raise NotImplementedError(f"--model {args.model}: only 'UnetConvNext' is built (UnetResNetBlock is not part of this package)")


# ===================================================================================================
# Trainer
# ===================================================================================================
CENTER_ONLY = Recipe('Dataset', 'none', 'center', False)          # diffusion.py:510-515: CenterCrop(image_size), ToTensor, t * 2 - 1


def _square(image_size):
    if isinstance(image_size, (tuple, list)):
        if len(image_size) != 2 or image_size[0] != image_size[1]:
            raise NotImplementedError(f"image_size={image_size}: the device input pipeline crops square images")
        return int(image_size[0])
    return int(image_size)


class DecolorTrainer(Trainer):
    """diffusion.py:563-760 on the shared Trainer (fused gradient accumulation, flat Adam / EMA, device image cache).  The default dataset
    chain is `CenterCrop(image_size)` on the file's own size; `to_lab=True` converts every batch with `cdf_lab_convert`; `random_aug`
    (RandomResizedCrop -> mirror -> RandomApply([ColorJitter])) runs on the device image cache in one launch per batch
    (`cdf_augment_jitter_batch`, `data.RANDOM_AUG`) when `device_data` is on; with `device_data=False`, a folder the cache cannot hold,
    or `torchvision_dataset` (torchvision's dataset classes) it is the host `DataLoader`, which needs torchvision and raises an
    ImportError naming the option where that is missing."""
    image_size_from_model = False
    force_shuffle = True

    @staticmethod
    def recipe_for(dataset):
        return CENTER_ONLY

    def __init__(self, diffusion_model, folder, *, ema_decay=0.995, image_size=128, train_batch_size=32, train_lr=2e-5,
                 train_num_steps=100000, gradient_accumulate_every=2, fp16=False, step_start_ema=2000, update_ema_every=10,
                 save_and_sample_every=5000, save_with_time_stamp_every=50000, results_folder='./results', load_path=None,
                 random_aug=False, torchvision_dataset=False, dataset=None, to_lab=False, order_seed=-1, num_workers=4, device_data=None):
        self.to_lab = to_lab
        self.order_seed = int(order_seed)
        self.random_aug = random_aug
        self.torchvision_dataset = torchvision_dataset
        self.save_with_time_stamp_every = save_with_time_stamp_every
        self.num_timesteps = diffusion_model.num_timesteps
        self.post_process_func = rgb2lab if to_lab else (lambda x: x)
        Path(results_folder).mkdir(parents=True, exist_ok=True)
        if image_size == 256 or (isinstance(image_size, (tuple, list)) and image_size[0] == 256):
            raise NotImplementedError("image_size 256 (CenterCrop(128) + Resize) is not built")
        if torchvision_dataset:
            device_data = False                     # (torchvision's dataset classes are host objects; `random_aug` alone runs on the device)
        super().__init__(diffusion_model, folder, ema_decay=ema_decay, image_size=_square(image_size), train_batch_size=train_batch_size,
                         train_lr=train_lr, train_num_steps=train_num_steps, gradient_accumulate_every=gradient_accumulate_every, fp16=fp16,
                         step_start_ema=step_start_ema, update_ema_every=update_ema_every, save_and_sample_every=save_and_sample_every,
                         results_folder=results_folder, load_path=load_path, dataset=dataset, shuffle=True, num_workers=num_workers,
                         device_data=device_data)
        self.image_size = diffusion_model.image_size if not hasattr(diffusion_model, 'module') else diffusion_model.module.image_size

    def _make_loader(self, folder, dataset, shuffle, num_workers, seed):
        if not (self.random_aug or self.torchvision_dataset):
            return super()._make_loader(folder, dataset, shuffle, num_workers, seed)
        if self.random_aug and not self.torchvision_dataset and self.device_data and folder is not None and dataset != 'synthetic':
            # the unresized RGB folder in HBM; RandomResizedCrop / mirror / ColorJitter / ToTensor per batch in one launch
            self.recipe = RANDOM_AUG
            try:
                cache = DeviceImageCache(folder, self.data_image_size, self.device, recipe=RANDOM_AUG)
                return cache, DeviceLoader(cache, self.batch_size, shuffle=True, seed=seed, rank=parallel.rank(), world=parallel.world_size(),
                                           drop_last=self.drop_last or parallel.world_size() > 1)
            except CacheUnfit as e:
                print(f"device image cache not used ({e}); falling back to the host DataLoader")
                self.device_data = False
        option = 'torchvision_dataset=True' if self.torchvision_dataset else 'random_aug=True'
        try:
            import torchvision                                                   # noqa: F401
        except ImportError as e:
            raise ImportError(f"Trainer({option}) needs torchvision (its dataset classes / ColorJitter / RandomResizedCrop), which is not "
                              f"installed; the default CenterCrop chain runs without it") from e
        from torch.utils import data
        from . import decolor_data
        size = (self.data_image_size, self.data_image_size)
        if self.torchvision_dataset:
            ds = decolor_data.get_dataset(dataset, folder, size, random_aug=self.random_aug)
        else:
            ds = decolor_data.FolderDataset(folder, size, random_aug=self.random_aug)
        dl = cycle(data.DataLoader(ds, batch_size=self.batch_size, shuffle=True, pin_memory=self.device.type == 'cuda',
                                   num_workers=num_workers))
        self.drop_last = False                                                   # (the host loader may end an epoch on a short batch)
        return ds, dl

    def _process_item(self, x):
        f = self.post_process_func
        return f(x[0]) if type(x) == list else f(x)

    def _next_batch(self):
        return self.post_process_func(super()._next_batch())

    # -- the reference Trainer's evaluation scripts (diffusion.py:764-959, 1000-1145) -------------------------------------------------------
    # The shared EvalMixin methods of the same names are written against the other packages' sampler return values; these follow this
    # package's upstream: names, arguments, file names and print wording.  Titles (add_title: cv2 text) are left out.
    def _write_image(self, tensor, path, nrow=8):
        """The one place an evaluation image reaches a file: a ready [C,H,W] grid as it is, a [B,C,H,W] batch through `save_image`."""
        if tensor.dim() == 3:
            write_grid(tensor.detach().float().cpu(), path)
        else:
            save_image(tensor, path, nrow=nrow)

    def shift_data_range(self, img):
        return (img + 1.0) / 2

    def save_og_test(self, og_dict, extra_path):
        for k, img in og_dict.items():
            img_grid = make_grid((img + 1) * 0.5, nrow=6)
            self._write_image(img_grid, str(self.results_folder / f'{k}-{extra_path}.png'))
            og_dict[k] = img_grid

    def save_gif(self, X_0s, X_ts, extra_path, init_recon=None, og=None):
        """Per step the x0 and x_t grids, nested as upstream nests them -- (frame grid, og grid [, init_recon grid]) -- as PNGs, and the
        two GIFs of those files (through PIL; upstream: imageio)."""
        from PIL import Image
        if init_recon is not None:
            init_recon = (init_recon + 1) * 0.5
        self.gif_len = len(X_0s)

        def nested(batch):
            grid = make_grid((batch + 1) * 0.5, nrow=6)
            if init_recon is not None:
                return make_grid(torch.stack((grid, og, make_grid(init_recon, nrow=6))), nrow=3)
            if og is not None:
                return make_grid(torch.stack((grid, og)), nrow=2)
            return grid

        frames_0, frames_t = [], []
        for i in range(len(X_0s)):
            print(i)
            for frames, batch, tag in ((frames_0, X_0s[i], 'x0'), (frames_t, X_ts[i], 'xt')):
                path = str(self.results_folder / f'sample-{i}-{extra_path}-{tag}.png')
                self._write_image(nested(batch), path)
                frames.append(path)
        for tag, frames in (('x0', frames_0), ('xt', frames_t)):
            ims = [Image.open(f).convert('RGB') for f in frames]
            if ims:
                ims[0].save(str(self.results_folder / f'Gif-{extra_path}-{tag}.gif'), save_all=True, append_images=ims[1:], duration=100, loop=0)

    def test_from_data(self, extra_path, s_times=None):
        """The first batch of the loader (upstream returns after it): og grid, per-step grids, GIFs."""
        og_img = self._next_batch()
        og_dict = {'og': og_img}
        X_0s, X_ts, init_recon, img_forward_list = self.ema_core.all_sample(batch_size=self.batch_size, img=og_img, times=s_times,
                                                                            res_dict=og_dict)
        og_dict['og'] = og_img.cpu()
        print('Generating on batch 0')
        self.save_og_test(og_dict, extra_path)
        self.save_gif(X_0s, X_ts, extra_path, init_recon=init_recon, og=og_dict['og'])

    def test_with_mixup(self, extra_path):
        og_img_1 = self._next_batch()
        og_img_2 = self._next_batch()
        og_img = (og_img_1 + og_img_2) / 2
        # (upstream unpacks two values from all_sample's four -- a ValueError there; the evident intent)
        X_0s, X_ts = self.ema_core.all_sample(batch_size=self.batch_size, img=og_img)[:2]
        print('Finish sample generation')
        og_dict = {'og1': og_img_1, 'og2': og_img_2, 'og': og_img}
        self.save_og_test(og_dict, extra_path)
        self.save_gif(X_0s, X_ts, extra_path, og=og_dict['og'])

    def test_from_random(self, extra_path):
        og_img = self._next_batch() * 0.9
        og_dict = {'og': og_img}
        X_0s, X_ts = self.ema_core.all_sample(batch_size=self.batch_size, img=og_img, res_dict=og_dict)[:2]       # (as test_with_mixup)
        print('Finish sample generation')
        self.save_og_test(og_dict, extra_path)
        self.save_gif(X_0s, X_ts, extra_path, og=og_dict['og'])

    def paper_invert_section_images(self, s_times=None, rounds=20):
        """Per round one batch; per window j of B // 9 the 3-column grids of og[j:j+9] / X_0s[0] / X_0s[-1] / X_ts[0] (upstream's windows
        start at j, not 9 j: kept) and their montage all_{cnt}.png: each PNG in a 10-pixel black border, side by side (numpy / PIL)."""
        import numpy as np
        from PIL import Image
        cnt = 0
        for i in range(rounds):
            og_img = self._next_batch()
            print(og_img.shape)
            X_0s, X_ts, _, _ = self.ema_core.all_sample(batch_size=self.batch_size, img=og_img, times=s_times)
            og_img = (og_img + 1) * 0.5
            for j in range(og_img.shape[0] // 9):
                parts = (('original', og_img[j: j + 9]), ('direct_recons', (X_0s[0][j: j + 9] + 1) * 0.5),
                         ('sampling_recons', (X_0s[-1][j: j + 9] + 1) * 0.5), ('blurry_image', (X_ts[0][j: j + 9] + 1) * 0.5))
                for name, z in parts:
                    self._write_image(z, str(self.results_folder / f'{name}_{cnt}.png'), nrow=3)
                framed = []
                for name in ('blurry_image', 'direct_recons', 'sampling_recons', 'original'):
                    a = np.asarray(Image.open(str(self.results_folder / f'{name}_{cnt}.png')).convert('RGB'))
                    framed.append(np.pad(a, ((10, 10), (10, 10), (0, 0))))
                Image.fromarray(np.concatenate(framed, axis=1)).save(str(self.results_folder / f'all_{cnt}.png'))
                cnt += 1

    def fid_distance_decrease_from_manifold(self, fid_func, start=0, end=1000, eval_batch_size=16, shard=False, lpips=None):
        """Degrade -> restore the dataset items idx with start < idx <= end of a `np.random.permutation` walk (numpy's global stream, as
        upstream); RMSE / SSIM (/ FID when fid_func is given) of the degraded, the sampled and the directly reconstructed sets against
        the originals.  The items are the dataset's own (upstream does not pass them through `post_process_func`: with `to_lab` the
        network is fed RGB -- reproduced).  The sampler runs in its ends-only mode and the two metrics accumulate per batch
        (`metrics.PairStats`: one launch per batch, one host read at the end); the four sets are kept, on the device, only for a plain
        fid_func.  A fid_func with `new_stats` / `kid` / `prdc`, `shard` and `lpips` are those of `EvalMixin`'s sweep of the same name
        (`metrics.SweepStats`); sharded, the ranks walk rank 0's permutation (every rank still draws its own, so its numpy stream
        advances as without the keyword).
        -> the numbers upstream prints."""
        import numpy as np
        rank, world, say = sweep_ranks(fid_func, shard, lpips)
        say(len(self.ds))
        perp = np.random.permutation(len(self.ds))
        if world > 1:
            walk = torch.from_numpy(perp).to(self.device)
            torch.distributed.broadcast(walk, src=0)
            perp = walk.cpu().numpy()

        def progress(idx, last):
            if idx % 1000 == 0:
                say(idx)
            if last:
                say(idx)

        all_samples = self._dataset_rows(start, end, every=True, fetch=lambda idx: self._dataset_item(int(perp[idx])), seen=progress)
        names = ('blur', 'deblur', 'direct_deblur')
        stats = metrics.SweepStats(names, fid_func, lpips, keep=fid_func is not None and not hasattr(fid_func, 'new_stats'))
        shape = None                                           # (a rank whose share is empty never sees one; rank 0, which prints, has batch 0)
        for k, og_img in enumerate(all_samples.split(eval_batch_size)):
            if k % world != rank:
                continue
            og_img = og_img.float()
            say(og_img.shape)
            xt, direct, final = self.ema_core.all_sample(batch_size=og_img.shape[0], img=og_img, times=None, ends_only=True)
            sets = [og_img, xt, final, direct]
            if og_img.shape[2] > 256:
                sets = [nn.functional.interpolate(z, size=64) for z in sets]
            sets = [rep3(z) for z in sets]
            stats.add(sets)
            shape = sets[0].shape[1:]
        if world > 1:
            stats.all_reduce(self.device)
        out = stats.pairs.result()
        if lpips is not None:
            out.update(stats.lstats.result())
        if stats.sets is not None:
            for z in stats.kept():
                print(z.shape)
        if stats.fstats and rank == 0:
            for st in stats.fstats:
                print(torch.Size((st.n, *shape)))
        for k, (name, word) in enumerate(zip(names, ('blurry', 'deblurred', 'direct deblurred'))):
            if fid_func is not None:
                out[f'fid_{name}'] = stats.fid(k)
                say(metrics.metric_line('FID', word, out[f'fid_{name}']))
            if stats.has_kid:
                out[f'kid_{name}'], out[f'kid_std_{name}'] = stats.kid(k)
                say(metrics.metric_line('KID', word, out[f'kid_{name}'], out[f'kid_std_{name}']))
            if stats.has_prdc:
                prdc = stats.prdc(k)
                metrics.put_prdc(out, name, prdc)
                say(metrics.prdc_line(word, prdc))
            say(metrics.metric_line('RMSE', word, out[f'rmse_{name}']))
            say(metrics.metric_line('SSIM', word, out[f'ssim_{name}']))
            if lpips is not None:
                say(metrics.metric_line('LPIPS', word, out[f'lpips_{name}']))
            if fid_func is not None and name != 'blur':
                say(metrics.fid_gain_line(out, name))
        return out

    # figure code (cv2 text, matplotlib) and the two methods that are dead upstream (`metrics` is never imported there): closed, with the
    # reference's signatures
    def _not_built(self, *a, **k):
        raise NotImplementedError("the figure methods of the decolorization Trainer are not built")

    def add_title(self, path, title_texts):
        return self._not_built()

    def make_transparent(self, path):
        return self._not_built()

    def create_metric_dict(self):
        return self._not_built()

    def save_metric(self, metric_dict, prefix=''):
        return self._not_built()

    def paper_showing_diffusion_images(self, s_times=None):
        return self._not_built()

    def paper_showing_diffusion_images_cover_page(self):
        return self._not_built()

    NOT_BUILT = ("add_title", "make_transparent", "create_metric_dict", "save_metric", "paper_showing_diffusion_images",
                 "paper_showing_diffusion_images_cover_page")

    def save(self, save_with_time_stamp=False):
        if parallel.rank() != 0:
            return
        ckpt = {'step': self.step, 'model': self.model.state_dict(), 'ema': self.ema_model.state_dict()}
        name = f'model_{self.step}.pt' if save_with_time_stamp else 'model.pt'
        torch.save(ckpt, str(self.results_folder / name))

    def train(self):
        while self.step < self.train_num_steps:
            loss = self.train_step()
            if not self.quiet and parallel.rank() == 0 and self.step % 100 == 0:
                print(f'{self.step}: {loss.item()}')
            if self.step != 0 and self.step % self.save_and_sample_every == 0:
                if parallel.rank() == 0:
                    milestone = self.step // self.save_and_sample_every
                    og_img = self._next_batch()
                    sample_dict = self.ema_core.sample(batch_size=og_img.shape[0], img=og_img)
                    if self.to_lab:
                        og_img = lab2rgb(og_img)
                    sample_dict['og'] = og_img
                    print(f'images saved: {sample_dict.keys()}')
                    for k, img in sample_dict.items():
                        save_image((img + 1) * 0.5, str(self.results_folder / f'sample-{k}-{milestone}.png'), nrow=6)
                    self.save()
                parallel.milestone_barrier()
            if self.step != 0 and self.step % self.save_with_time_stamp_every == 0:
                self.save(save_with_time_stamp=True)
            self.step += 1
