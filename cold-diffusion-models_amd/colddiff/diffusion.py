"""The four `GaussianDiffusion` classes of the cold-diffusion packages, on the HIP degradation kernels.

Constructor arguments, attribute names, method names, return values and `state_dict` layout follow
  deblurring  : deblurring_diffusion_pytorch.py:311-981
  denoising   : denoising_diffusion_pytorch.py:310-542
  resolution  : resolution_diffusion_pytorch.py:325-767
  defading    : defading_diffusion_gaussian.py:298-554
What differs is the execution: q_sample and every Alg.1/Alg.2 sampler step is ONE fused kernel
launch (the whole step chain runs with the image plane resident in LDS) instead of O(T) convs, a
torch.stack of T images and B python-level gathers, and nothing synchronises with the host
(the reference's `torch.max(t)` -> `range()` does).
"""
import numpy as np
import torch
from torch import nn

from . import degrade as D
from . import runtime as rt
from .graphsample import SampleGraphMixin


def _full_step(batch_size, value, device):
    return torch.full((batch_size,), value, dtype=torch.long, device=device)


# ===================================================================================================
# deblurring
# ===================================================================================================
class TwoPhase(SampleGraphMixin):
    """forward() in two phases -- prepare() draws t exactly as forward() does and runs the degradation, loss_prepared() runs the
    network and the loss: prepare + loss_prepared == forward, same draws in the same order, same kernels.  The Trainer uses it to
    (a) degrade the next micro-batch on a side stream under the current forward / backward (deblurring) and (b) run the
    `gradient_accumulate_every` micro-batches of an optimizer step as ONE pass of the network (`Trainer._can_fuse`): the loss of the
    concatenated batch is the mean of the micro-batch losses, so its gradient is the sum of the (loss_i / accumulate).backward() calls
    of DEBLUR:1188-1195 -- nothing in these networks couples samples (channel LayerNorm is per pixel, GroupNorm per sample)."""

    def fusable(self):
        return getattr(self, 'train_routine', 'Final') == 'Final'

    def graph_safe(self):
        """True only where prepare() (the draw of t and q_sample) never reads a device value on the host and takes nothing else from
        the host that changes from step to step: then the Trainer may capture the step into a graph.  A core that was not checked
        says False."""
        return False

    def _draw_t(self, x):
        b, c, h, w = x.shape
        assert h == self.image_size and w == self.image_size, f'height and width of image must be {self.image_size}'
        return torch.randint(0, self.num_timesteps, (b,), device=x.device).long()

    def _network(self):
        return self.defade_fn if hasattr(self, 'defade_fn') else self.denoise_fn

    def prepare(self, x, x2=None, t=None):
        """-> (target, t, degraded input): what p_losses hands to the network and to the loss ('Final' training routine)."""
        assert self.fusable()
        if t is None:
            t = self._draw_t(x)
        return x, t, (self.q_sample(x_start=x, t=t) if x2 is None else self.q_sample(x_start=x, x_end=x2, t=t))

    def loss_prepared(self, prep):
        x_start, t, x_deg = prep
        return D.loss(x_start, self._network()(x_deg, t), self.loss_type)


class DeblurDiffusion(TwoPhase, nn.Module):
    def __init__(self, denoise_fn, *, image_size, device_of_kernel, channels=3, timesteps=1000, loss_type='l1', kernel_std=0.1,
                 kernel_size=3, blur_routine='Incremental', train_routine='Final', sampling_routine='default', discrete=False):
        super().__init__()
        self.channels = channels
        self.image_size = image_size
        self.denoise_fn = denoise_fn
        self.device_of_kernel = device_of_kernel
        self.num_timesteps = int(timesteps)
        self.loss_type = loss_type
        self.kernel_std = kernel_std
        self.kernel_size = kernel_size
        self.blur_routine = blur_routine
        self.gaussian_kernels = nn.ModuleList(self.get_kernels())
        self.train_routine = train_routine
        self.sampling_routine = sampling_routine
        self.discrete = discrete
        self._taps_cache = None

    # -- kernel construction (DEBLUR:348-389) -------------------------------------------------------
    def blur(self, dims, std):
        return D.gaussian_kernel2d(dims, std)

    def get_conv(self, dims, std, mode='circular'):
        kernel = self.blur(dims, std)
        conv = nn.Conv2d(in_channels=self.channels, out_channels=self.channels, kernel_size=dims, padding=int((dims[0] - 1) / 2),
                         padding_mode=mode, bias=False, groups=self.channels)
        with torch.no_grad():
            conv.weight = nn.Parameter(kernel[None, None].repeat(self.channels, 1, 1, 1))
        return conv

    def get_kernels(self):
        kernels, ks, std = [], self.kernel_size, self.kernel_std
        for i in range(self.num_timesteps):
            r = self.blur_routine
            if r == 'Incremental':
                kernels.append(self.get_conv((ks, ks), (std * (i + 1), std * (i + 1))))
            elif r == 'Constant':
                kernels.append(self.get_conv((ks, ks), (std, std)))
            elif r == 'Constant_reflect':
                kernels.append(self.get_conv((ks, ks), (std, std), mode='reflect'))
            elif r == 'Exponential_reflect':
                kstd = np.exp(std * i)
                kernels.append(self.get_conv((ks, ks), (kstd, kstd), mode='reflect'))
            elif r == 'Exponential':
                kstd = np.exp(std * i)
                kernels.append(self.get_conv((ks, ks), (kstd, kstd)))
            elif r == 'Individual_Incremental':
                k = 2 * i + 1
                kernels.append(self.get_conv((k, k), (2 * k, 2 * k)))
            elif r == 'Special_6_routine':
                kstd = i / 100 + 0.35
                kernels.append(self.get_conv((11, 11), (kstd, kstd), mode='reflect'))
        return kernels

    # -- fused application of the kernel stack -----------------------------------------------------------
    def _pad_mode(self):
        return D.PAD_MODES[self.gaussian_kernels[0].padding_mode]

    def _uniform(self):
        return self.blur_routine != 'Individual_Incremental'

    def _taps(self, device):
        """[T, C, k, k] stack of the (state_dict) kernel weights on the image's device."""
        ws = [m.weight for m in self.gaussian_kernels]
        key = (str(device), tuple((w.data_ptr(), w._version) for w in ws))
        if self._taps_cache is None or self._taps_cache[0] != key:
            taps = torch.stack([w.detach()[:, 0] for w in ws]).to(device).contiguous()
            self._taps_cache = (key, taps, D.separable_taps(taps))
        return self._taps_cache[1]

    def _taps1d(self, device):
        """[T, C, 2, k] 1-D factors of the kernels when all of them are rank one (the Gaussians are), else None."""
        self._taps(device)
        return self._taps_cache[2]

    def _apply_one(self, i, x):
        """gaussian_kernels[i](x) (any kernel size)."""
        m = self.gaussian_kernels[i]
        k = m.weight.shape[-1]
        return D.blur_step(x, m.weight.detach()[:, 0].contiguous(), k, D.PAD_MODES[m.padding_mode])

    def _degrade(self, x, nsteps, t=None, img=None, want_prev=False, quantise=False):
        """D(x, nsteps): kernels 0..nsteps-1 (or 0..t[b] per sample), discrete mean-collapse included."""
        _, _, H, W = x.shape
        collapse = self.num_timesteps - 1 if self.discrete else -1
        if self._uniform() and D.blur_fits_lds(H, W, self.gaussian_kernels[0].weight.shape[-1]):
            k = self.gaussian_kernels[0].weight.shape[-1]
            return D.blur_chain(x, self._taps(x.device), k, self._pad_mode(), t=t, step_lo=0, step_hi=nsteps - 1, img=img,
                                want_prev=want_prev, collapse_step=collapse, quantise=quantise, taps1d=self._taps1d(x.device))
        assert t is None and not quantise, "per-sample t needs the LDS-resident path"
        prev = x
        for i in range(nsteps):
            prev = x
            x = self._apply_one(i, x)
            if i == collapse:
                x = D.plane_mean_(x)
        if img is not None:
            return D.x0_step_down(img, x, prev)
        return (x, prev) if want_prev else x

    def _collapse(self, img):
        return D.plane_mean_(img.clone()) if self.discrete else img

    # -- samplers (DEBLUR:393-689) --------------------------------------------------------------------
    def _forward_process(self, img, t):
        if self.blur_routine == 'Individual_Incremental':
            return self._apply_one(t - 1, img)
        saved, self.discrete = self.discrete, False          # the forward pass never mean-collapses inside the loop
        try:
            return self._degrade(img, t)
        finally:
            self.discrete = saved

    def _reverse_step(self, img, x, t):
        if self.sampling_routine == 'default':
            if self.blur_routine == 'Individual_Incremental':
                return self._apply_one(t - 2, x)
            saved, self.discrete = self.discrete, False      # Alg.1 chain has no collapse (DEBLUR:432-434)
            try:
                return self._degrade(x, t - 1)
            finally:
                self.discrete = saved
        if self.sampling_routine == 'x0_step_down':
            return self._degrade(x, t, img=img)              # img - D(x,t) + D(x,t-1)
        return x

    # -- sampler graph mode (graphsample.py): the reverse step with every `t` read from the step table -------------------
    def _sg_why(self):
        if not self._uniform():
            return "blur_routine='Individual_Incremental' applies one kernel per step, picked by a host index"
        if not D.blur_fits_lds(self.image_size, self.image_size, self.gaussian_kernels[0].weight.shape[-1]):
            return "the plane is past the LDS cap: the per-step blur fallback takes host step counts"
        if self.train_routine != 'Final':
            return "train_routine is not 'Final'"
        return None

    def _sg_step(self, cur, tb):
        x = self.denoise_fn(cur, tb.step)
        if self.sampling_routine == 'default':
            saved, self.discrete = self.discrete, False      # (as _reverse_step)
            try:
                return x, self._degrade(x, 0, t=tb.prev)      # D(x, t - 1): row -1 is the identity
            finally:
                self.discrete = saved
        if self.sampling_routine == 'x0_step_down':
            return x, self._degrade(x, 0, t=tb.step, img=cur)
        return x, x

    @torch.no_grad()
    def _sample_impl(self, batch_size, img, t, noise_level, graph=None):
        self.denoise_fn.eval()
        if t is None:
            t = self.num_timesteps
        img = self._forward_process(rt.check(img), t)
        img = self._collapse(img)
        if noise_level is not None:
            img = img + torch.randn_like(img) * noise_level
        xt = img
        direct_recons, img = self._reverse_loop(batch_size, img, t, graph)
        return xt, direct_recons, img

    def _reverse_loop(self, batch_size, img, t, graph=None):
        direct_recons = None
        sg = self._sg(graph)
        if sg is not None:
            done = sg.reverse('reverse', self._sg_step, img, t, batch_size, why=self._sg_why())
            if done is not None:
                direct_recons, img, t, _ = done
        while t:
            step = _full_step(batch_size, t - 1, img.device)
            x = self.denoise_fn(img, step)
            if self.train_routine == 'Final':
                if direct_recons is None:
                    direct_recons = x
                x = self._reverse_step(img, x, t)
            img = x
            t = t - 1
        return direct_recons, img

    def sample(self, batch_size=16, img=None, t=None, graph=None):
        out = self._sample_impl(batch_size, img, t, None, graph)
        self.denoise_fn.train()
        return out

    def gen_sample(self, batch_size=16, img=None, t=None, noise_level=0, graph=None):
        return self._sample_impl(batch_size, img, t, noise_level, graph)

    gen_sample_2 = gen_sample

    def _chain(self, x, n, img=None, collapse=True):
        """Kernels 0..n-1 on x (with img: the Alg.2 combination); `collapse=False` drops the discrete mean-collapse."""
        saved, self.discrete = self.discrete, self.discrete and collapse
        try:
            return self._degrade(x, n, img=img)
        finally:
            self.discrete = saved

    def _trajectory(self, img, lo, hi):
        """[K_lo(img), K_{lo+1}(K_lo(img)), ...] for kernels lo..hi-1, one launch per step (any kernel size)."""
        out = []
        for i in range(lo, hi):
            img = self._apply_one(i, img)
            out.append(img)
        return out

    @torch.no_grad()
    def forward_and_backward(self, batch_size=16, img=None, noise_level=0, t=None, times=None, eval=True, graph=None):
        """The whole forward trajectory and every x_t on the way back (DEBLUR:692-770)."""
        self._sg_eager(graph, "forward_and_backward keeps every step's image: not captured")
        if eval:
            self.denoise_fn.eval()
        if t is None:
            t = self.num_timesteps
        if times is None:
            times = t
        img = rt.check(img)
        Forward = [img]
        individual = self.blur_routine == 'Individual_Incremental'
        if individual:
            img = self._apply_one(t - 1, img)
        else:
            Forward += self._trajectory(img, 0, t)
            img = Forward[-1]
        Backward = []
        if self.discrete:
            img = self._collapse(img)
            img = img + torch.randn_like(img) * noise_level
        while times:
            step = _full_step(batch_size, times - 1, img.device)
            x = self.denoise_fn(img, step)
            Backward.append(img)
            if self.train_routine == 'Final':
                if individual:
                    if self.sampling_routine in ('default', 'x0_step_down') and times - 2 >= 0:
                        x = self._apply_one(times - 2, img)           # reference quirk: blurs x_t (DEBLUR:731-733, 744-746)
                elif self.sampling_routine == 'default':
                    x = self._chain(x, times - 1, collapse=False)
                elif self.sampling_routine == 'x0_step_down':
                    x = self._chain(x, times, img=img)
            img = x
            times = times - 1
        return Forward, Backward, img

    @torch.no_grad()
    def forward_and_backward_2(self, batch_size=16, img=None, noise_level=0, eval=True, graph=None):
        """One forward trajectory, then back twice from the same x_T: with D(x0_hat, t-1) (written `img - img + ...`
        upstream) and with Algorithm 2 (DEBLUR:773-861)."""
        self._sg_eager(graph, "forward_and_backward_2 keeps every step's image: not captured")
        if eval:
            self.denoise_fn.eval()
        T = self.num_timesteps
        img = rt.check(img)
        Forward = [img] + self._trajectory(img, 0, T)
        img = Forward[-1]
        if self.discrete:
            img = self._collapse(img)
            img = img + torch.randn_like(img) * noise_level
        last_img = img
        runs = []
        for alg2 in (False, True):
            img, times, back = last_img, T, []
            while times:
                step = _full_step(batch_size, times - 1, img.device)
                x = self.denoise_fn(img, step)
                back.append(img)
                img = self._chain(x, times, img=img) if alg2 else self._chain(x, times - 1, collapse=False)
                times = times - 1
            runs.append((back, img))
        return Forward, runs[0][0], runs[1][0], runs[0][1], runs[1][1]

    @torch.no_grad()
    def sample_from_blur(self, batch_size=16, img=None, t=None, times=None, eval=True, start=None, graph=None):
        """`sample` for an input that already carries kernels 0..start-1 (DEBLUR:864-925)."""
        if eval:
            self.denoise_fn.eval()
        if t is None:
            t = self.num_timesteps
        if start is None:
            start = 0
        img = rt.check(img)
        H, W = img.shape[2:]
        k = self.gaussian_kernels[0].weight.shape[-1]
        if t > start and self._uniform() and D.blur_fits_lds(H, W, k):
            img = D.blur_chain(img, self._taps(img.device), k, self._pad_mode(), step_lo=start, step_hi=t - 1,
                               taps1d=self._taps1d(img.device))
        else:
            for i in range(start, t):
                img = self._apply_one(i, img)
        img = self._collapse(img)
        xt = img
        direct_recons, img = self._reverse_loop(batch_size, img, t, graph)
        return xt, direct_recons, img

    @torch.no_grad()
    def opt(self, img, t=None):
        if t is None:
            t = self.num_timesteps
        return self._forward_process(rt.check(img), t)

    @torch.no_grad()
    def all_sample(self, batch_size=16, img=None, t=None, times=None, eval=True, graph=None):
        if eval:
            self.denoise_fn.eval()
        if t is None:
            t = self.num_timesteps
        if times is None:
            times = t
        img = self._forward_process(rt.check(img), t)
        X_0s, X_ts = [], []
        noise = None
        if self.discrete:
            img = self._collapse(img)
            noise = torch.randn_like(img) * 0.001
            img = img + noise
        sg = self._sg(graph)
        if sg is not None:
            done = sg.reverse('all_sample', self._sg_step, img, times, batch_size, put='cur', why=self._sg_why())
            if done is not None:
                _, img, times, (X_0s, X_ts) = done
        while times:
            step = _full_step(batch_size, times - 1, img.device)
            x = self.denoise_fn(img, step)
            X_0s.append(x)
            X_ts.append(img)
            if self.train_routine == 'Final':
                if self.blur_routine == 'Individual_Incremental':
                    if times - 2 >= 0:
                        x = self._apply_one(times - 2, img)       # reference quirk: blurs x_t (DEBLUR:645-647)
                else:
                    x = self._reverse_step(img, x, times)
            img = x
            times = times - 1
        if self.discrete:
            img = img - noise
        X_0s.append(img)
        self.denoise_fn.train()
        return X_0s, X_ts

    # -- training (DEBLUR:927-981) --------------------------------------------------------------------------
    def q_sample(self, x_start, t):
        x_start = rt.check(x_start)
        if self._uniform() and D.blur_fits_lds(x_start.shape[2], x_start.shape[3], self.gaussian_kernels[0].weight.shape[-1]):
            return self._degrade(x_start, 0, t=t.contiguous(), quantise=self.discrete)
        # per-step fallback (varying kernel size / planes larger than LDS): blur to max(t), pick per sample
        max_iters = int(torch.max(t))
        x, out = x_start, torch.empty_like(x_start)
        for i in range(max_iters + 1):
            x = self._apply_one(i, x)
            if self.discrete and i == self.num_timesteps - 1:
                x = D.plane_mean_(x)
            sel = (t == i).view(-1, 1, 1, 1)
            out = torch.where(sel, x, out)
        if self.discrete:
            out = ((out + 1) * 0.5 * 255).int().float() / 255 * 2 - 1
        return out

    def p_losses(self, x_start, t):
        if self.train_routine == 'Final':
            x_blur = self.q_sample(x_start=x_start, t=t)
            x_recon = self.denoise_fn(x_blur, t)
            return D.loss(x_start, x_recon, self.loss_type)
        raise NotImplementedError()

    def forward(self, x, *args, **kwargs):
        b, c, h, w, device, img_size = *x.shape, x.device, self.image_size
        assert h == img_size and w == img_size, f'height and width of image must be {img_size}'
        t = torch.randint(0, self.num_timesteps, (b,), device=device).long()
        return self.p_losses(x, t, *args, **kwargs)

    # -- forward() in two phases, for the Trainer's degradation prefetch: the blur chain of micro-batch i+1 (up to T sequential
    # steps on B*C planes: 96 of 256 CUs at B = 32) does not depend on the network and runs on a side stream under the
    # forward / backward of micro-batch i.  prepare() + loss_prepared() == forward(): same draws, same kernels.
    def can_prepare_async(self):
        """True when q_sample is ONE sync-free launch (uniform kernel size, plane fits the LDS): only then does a side-stream
        prefetch overlap with anything -- the per-step fallback reads max(t) on the host and would block the launching thread."""
        return self._uniform() and D.blur_fits_lds(self.image_size, self.image_size, self.gaussian_kernels[0].weight.shape[-1])

    def graph_safe(self):
        """Exactly when q_sample is the one fused launch: t is a device draw and the per-step fallback's int(torch.max(t)) is not reached."""
        return self.can_prepare_async()


# ===================================================================================================
# denoising ("hot" Gaussian-noise baseline with cold-style samplers)
# ===================================================================================================
def cosine_beta_schedule(timesteps, s=0.008):
    steps = timesteps + 1
    x = torch.linspace(0, steps, steps)
    alphas_cumprod = torch.cos(((x / steps) + s) / (1 + s) * torch.pi * 0.5) ** 2
    alphas_cumprod = alphas_cumprod / alphas_cumprod[0]
    betas = 1 - (alphas_cumprod[1:] / alphas_cumprod[:-1])
    return torch.clip(betas, 0, 0.999)


class DenoiseDiffusion(TwoPhase, nn.Module):
    def __init__(self, denoise_fn, *, image_size, channels=3, timesteps=1000, loss_type='l1', train_routine='Final',
                 sampling_routine='default', discrete=False):
        super().__init__()
        self.channels = channels
        self.image_size = image_size
        self.denoise_fn = denoise_fn
        self.num_timesteps = int(timesteps)
        self.loss_type = loss_type
        betas = cosine_beta_schedule(timesteps)
        alphas_cumprod = torch.cumprod(1. - betas, axis=0)
        self.register_buffer('alphas_cumprod', alphas_cumprod)
        self.register_buffer('sqrt_alphas_cumprod', torch.sqrt(alphas_cumprod))
        self.register_buffer('sqrt_one_minus_alphas_cumprod', torch.sqrt(1. - alphas_cumprod))
        self.train_routine = train_routine
        self.sampling_routine = sampling_routine

    def _tables(self):
        return self.sqrt_alphas_cumprod, self.sqrt_one_minus_alphas_cumprod

    def q_sample(self, x_start, x_end, t):
        ca, cb = self._tables()
        return D.noise_qsample(rt.check(x_start), x_end, ca, cb, t.contiguous())

    def graph_safe(self):
        """t is a device draw; q_sample is one launch that gathers the schedule tables (buffers) by t on the device."""
        return True

    def get_x2_bar_from_xt(self, x1_bar, xt, t):
        ca, cb = self._tables()
        return (xt - ca.gather(-1, t).view(-1, 1, 1, 1) * x1_bar) / cb.gather(-1, t).view(-1, 1, 1, 1)

    @torch.no_grad()
    def _reverse(self, batch_size, img, t, est_noise, noise, graph=None):
        ca, cb = self._tables()
        direct_recons = None
        sg = self._sg(graph)
        if sg is not None:
            def step(cur, tb):
                x1_bar = self.denoise_fn(cur, tb.step)
                return x1_bar, D.noise_step_dev(cur, x1_bar, tb.st.get('noise'), ca, cb, tb.step, est_noise)
            done = sg.reverse(('reverse', est_noise), step, img, t, batch_size, st={'noise': noise})
            if done is not None:
                direct_recons, img, t, _ = done
        while t:
            step = _full_step(batch_size, t - 1, img.device)
            x1_bar = self.denoise_fn(img, step)
            if direct_recons is None:
                direct_recons = x1_bar
            img = D.noise_step(img, x1_bar, noise, ca, cb, t, est_noise)
            t = t - 1
        return direct_recons, img

    def sample(self, batch_size=16, img=None, t=None, graph=None):
        # always the estimated-noise form, whatever sampling_routine says (DENOISE:342-375)
        self.denoise_fn.eval()
        t = self.num_timesteps if t is None else t
        xt = rt.check(img)
        direct_recons, img = self._reverse(batch_size, xt, t, True, None, graph)
        self.denoise_fn.train()
        return xt, direct_recons, img

    def gen_sample(self, batch_size=16, img=None, t=None, graph=None):
        self.denoise_fn.eval()
        t = self.num_timesteps if t is None else t
        noise = rt.check(img)
        direct_recons = None
        if self.sampling_routine == 'ddim':
            direct_recons, img = self._reverse(batch_size, noise, t, True, None, graph)
        elif self.sampling_routine == 'x0_step_down':
            direct_recons, img = self._reverse(batch_size, noise, t, False, noise, graph)
        return noise, direct_recons, img

    @torch.no_grad()
    def forward_and_backward(self, batch_size=16, img=None, t=None, times=None, eval=True, graph=None):
        """Noising trajectory with ONE noise draw, then the fixed-noise way back (DENOISE:438-479)."""
        self._sg_eager(graph, "forward_and_backward keeps every step's image: not captured")
        self.denoise_fn.eval()
        t = self.num_timesteps if t is None else t
        ca, cb = self._tables()
        img = rt.check(img)
        Forward = [img]
        noise = torch.randn_like(img)
        for i in range(t):
            n_img = D.noise_qsample(img, noise, ca, cb, _full_step(batch_size, i, img.device))
            Forward.append(n_img)
        Backward, img = [], n_img
        while t:
            step = _full_step(batch_size, t - 1, img.device)
            x1_bar = self.denoise_fn(img, step)
            Backward.append(img)
            img = D.noise_step(img, x1_bar, noise, ca, cb, t, False)
            t = t - 1
        return Forward, Backward, img

    @torch.no_grad()
    def all_sample(self, batch_size=16, img=None, t=None, times=None, eval=True, graph=None):
        self._sg_eager(graph, "all_sample moves every step to the host, as upstream does")
        if eval:
            self.denoise_fn.eval()
        t = self.num_timesteps if t is None else t
        ca, cb = self._tables()
        X1_0s, X2_0s, X_ts = [], [], []
        while t:
            step = _full_step(batch_size, t - 1, img.device)
            x1_bar = self.denoise_fn(img, step)
            x2_bar = self.get_x2_bar_from_xt(x1_bar, img, step)
            X1_0s.append(x1_bar.detach().cpu())
            X2_0s.append(x2_bar.detach().cpu())
            X_ts.append(img.detach().cpu())
            img = D.noise_step(img, x1_bar, None, ca, cb, t, True)
            t = t - 1
        return X1_0s, X2_0s, X_ts

    def p_losses(self, x_start, x_end, t):
        if self.train_routine == 'Final':
            x_mix = self.q_sample(x_start=x_start, x_end=x_end, t=t)
            x_recon = self.denoise_fn(x_mix, t)
            return D.loss(x_start, x_recon, self.loss_type)
        raise NotImplementedError()

    def forward(self, x1, x2, *args, **kwargs):
        b, c, h, w, device, img_size = *x1.shape, x1.device, self.image_size
        assert h == img_size and w == img_size, f'height and width of image must be {img_size}'
        t = torch.randint(0, self.num_timesteps, (b,), device=device).long()
        return self.p_losses(x1, x2, t, *args, **kwargs)


# ===================================================================================================
# demixing: the cosine schedule blends an image of one dataset into an image of another
# (demixing-diffusion-pytorch/demixing_diffusion_pytorch/demixing_diffusion_pytorch.py:309-502 = DEMIX)
# ===================================================================================================
class DemixDiffusion(DenoiseDiffusion):
    """Same constructor, schedule, q_sample, p_losses, forward(x1, x2) and sample as the denoising class (the reference
    files differ only in the methods below, DEMIX vs DENOISE diff); `x2` is an image instead of Gaussian noise."""

    def gen_sample(self, batch_size=16, img=None, noise_level=0, t=None, graph=None):
        # always the fixed-x2 form, whatever sampling_routine says (DEMIX:384-413)
        self.denoise_fn.eval()
        t = self.num_timesteps if t is None else t
        noise = rt.check(img)
        img = noise + torch.randn_like(noise) * noise_level
        direct_recons, img = self._reverse(batch_size, img, t, False, noise, graph)
        return noise, direct_recons, img

    @torch.no_grad()
    def forward_and_backward(self, batch_size=16, img1=None, img2=None, t=None, times=None, eval=True, graph=None):
        """img1 mixed step by step into img2, then back with img2 held fixed (DEMIX:416-458)."""
        self._sg_eager(graph, "forward_and_backward keeps every step's image: not captured")
        self.denoise_fn.eval()
        t = self.num_timesteps if t is None else t
        ca, cb = self._tables()
        img, noise = rt.check(img1), rt.check(img2)
        Forward = [img]
        for i in range(t):
            n_img = D.noise_qsample(img, noise, ca, cb, _full_step(batch_size, i, img.device))
            Forward.append(n_img)
        Backward, img = [], n_img
        while t:
            step = _full_step(batch_size, t - 1, img.device)
            x1_bar = self.denoise_fn(img, step)
            Backward.append(img)
            img = D.noise_step(img, x1_bar, noise, ca, cb, t, False)
            t = t - 1
        return Forward, Backward, img

    def all_sample(self, batch_size=16, img=None, t=None, times=None, eval=True, graph=None):
        X1_0s, _, X_ts = super().all_sample(batch_size=batch_size, img=img, t=t, times=times, eval=eval, graph=graph)
        return X1_0s, X_ts                                            # (DEMIX:495)


# ===================================================================================================
# defading generation: per-pixel Gaussian-mask blend of an image into a second (solid-colour) image
# (defading-generation-diffusion-pytorch/defading_diffusion_pytorch/defading_diffusion_pytorch.py:309-568 = DEFGEN)
# ===================================================================================================
def get_fade_kernel(dims, std):                                       # DEFGEN:309-314
    k = D.gaussian_kernel2d(dims, std)
    k = k / torch.max(k)
    return (torch.ones_like(k) - k)[1:, 1:]


def get_kernels_with_schedule(timesteps, size, kernel_std, initial_mask):             # DEFGEN:316-324
    out, kers = [], torch.ones((1, size, size))
    for i in range(timesteps):
        kers = kers * get_fade_kernel((size + 1, size + 1), (kernel_std * (i + initial_mask), kernel_std * (i + initial_mask)))
        out.append(kers)
    return torch.stack(out)


def get_reverse_kernels_with_schedule(timesteps, size, kernel_std, initial_mask):     # DEFGEN:327-337
    out, kers = [], torch.ones((1, size, size))
    for i in range(timesteps):
        out.append(kers)
        kers = kers * get_fade_kernel((size + 1, size + 1), (kernel_std * (i + initial_mask), kernel_std * (i + initial_mask)))
    out.reverse()
    return torch.stack(out)


class DefadeGenDiffusion(TwoPhase, nn.Module):
    def __init__(self, denoise_fn, *, image_size, channels=3, timesteps=1000, loss_type='l1', train_routine='Final',
                 sampling_routine='default', reverse=False, kernel_std=0.15, initial_mask=11):
        super().__init__()
        self.channels = channels
        self.image_size = image_size
        self.denoise_fn = denoise_fn
        self.num_timesteps = int(timesteps)
        self.loss_type = loss_type
        self.reverse = reverse
        if self.reverse:
            one_minus_alphas = get_reverse_kernels_with_schedule(timesteps, image_size, kernel_std, initial_mask)
            alphas = 1. - one_minus_alphas
        else:
            alphas = get_kernels_with_schedule(timesteps, image_size, kernel_std, initial_mask)
            one_minus_alphas = 1. - alphas
        self.register_buffer('alphas', alphas)                       # [T, 1, H, W]
        self.register_buffer('one_minus_alphas', one_minus_alphas)
        self.train_routine = train_routine
        self.sampling_routine = sampling_routine

    def q_sample(self, x_start, x_end, t):
        return D.blend_qsample(rt.check(x_start), x_end, self.alphas, self.one_minus_alphas, t.contiguous())

    def get_x2_bar_from_xt(self, x1_bar, xt, t):
        return (xt - self.alphas[t] * x1_bar) / (self.one_minus_alphas[t] + 0.00000000000001)

    @torch.no_grad()
    def _reverse(self, batch_size, img, t, x2, collect=None, graph=None):
        direct_recons = None
        sg = self._sg(graph)
        if sg is not None:
            def step(cur, tb):
                x1_bar = self.denoise_fn(cur, tb.step)
                return x1_bar, D.blend_step_dev(cur, x1_bar, tb.st['x2'], self.alphas, self.one_minus_alphas, tb.step)
            done = sg.reverse('reverse', step, img, t, batch_size, st={'x2': x2},
                              why="every step's images are collected on the way: not captured" if collect is not None else None)
            if done is not None:
                direct_recons, img, t, _ = done
        while t:
            step = _full_step(batch_size, t - 1, img.device)
            x1_bar = self.denoise_fn(img, step)
            if direct_recons is None:
                direct_recons = x1_bar
            if collect is not None:
                collect(x1_bar, img)
            img = D.blend_step(img, x1_bar, x2, self.alphas, self.one_minus_alphas, t)
            t = t - 1
        return direct_recons, img

    def sample(self, batch_size=16, img=None, t=None, graph=None):   # DEFGEN:386-419 (x2 = the start image)
        self.denoise_fn.eval()
        t = self.num_timesteps if t is None else t
        xt = rt.check(img)
        direct_recons, img = self._reverse(batch_size, xt, t, xt, graph=graph)
        self.denoise_fn.train()
        return xt, direct_recons, img

    def gen_sample(self, batch_size=16, img=None, noise_level=0, t=None, graph=None):    # DEFGEN:428-457
        self.denoise_fn.eval()
        t = self.num_timesteps if t is None else t
        noise = rt.check(img)
        img = noise + torch.randn_like(noise) * noise_level
        direct_recons, img = self._reverse(batch_size, img, t, noise, graph=graph)
        return noise, direct_recons, img

    @torch.no_grad()
    def forward_and_backward(self, batch_size=16, img1=None, img2=None, t=None, times=None, eval=True, graph=None):   # DEFGEN:460-504
        self.denoise_fn.eval()
        t = self.num_timesteps if t is None else t
        img1, img2 = rt.check(img1), rt.check(img2)
        Forward = [img1]
        for i in range(self.num_timesteps):                          # (the whole schedule, whatever t says: DEFGEN:475)
            Forward.append(self.q_sample(img1, img2, _full_step(batch_size, i, img1.device)))
        Backward = []
        _, img = self._reverse(batch_size, img2, t, img2, collect=lambda x1, im: Backward.append(im), graph=graph)
        return Forward, Backward, img

    @torch.no_grad()
    def all_sample(self, batch_size=16, img=None, t=None, times=None, eval=True, graph=None):       # DEFGEN:507-541
        if eval:
            self.denoise_fn.eval()
        t = self.num_timesteps if t is None else t
        img = rt.check(img)
        X1_0s, X_ts = [], []
        self._reverse(batch_size, img, t, img, collect=lambda x1, im: (X1_0s.append(x1), X_ts.append(im)), graph=graph)
        return X1_0s, X_ts

    def p_losses(self, x_start, x_end, t):
        if self.train_routine == 'Final':
            x_mix = self.q_sample(x_start=x_start, x_end=x_end, t=t)
            x_recon = self.denoise_fn(x_mix, t)
            return D.loss(x_start, x_recon, self.loss_type)
        raise NotImplementedError()

    def forward(self, x1, x2, *args, **kwargs):
        b, c, h, w, device, img_size = *x1.shape, x1.device, self.image_size
        assert h == img_size and w == img_size, f'height and width of image must be {img_size}'
        t = torch.randint(0, self.num_timesteps, (b,), device=device).long()
        return self.p_losses(x1, x2, t, *args, **kwargs)


# ===================================================================================================
# resolution (pixelation)
# ===================================================================================================
class ResolutionDiffusion(TwoPhase, nn.Module):
    _MODES = {'': 'bicubic', '_bilinear': 'bilinear', '_area': 'area', '_bicubic': 'bicubic'}

    def __init__(self, denoise_fn, *, image_size, device_of_kernel, channels=3, timesteps=1000, loss_type='l1',
                 resolution_routine='Incremental', train_routine='Final', sampling_routine='default'):
        super().__init__()
        self.channels = channels
        self.image_size = image_size
        self.denoise_fn = denoise_fn
        self.device_of_kernel = device_of_kernel
        self.num_timesteps = int(timesteps)
        self.loss_type = loss_type
        self.resolution_routine = resolution_routine
        self.train_routine = train_routine
        self.sampling_routine = sampling_routine
        self._parse_routine()
        self.func = self.get_funcs()
        self._sizes_cache = {}

    def _parse_routine(self):
        r = self.resolution_routine
        assert r.startswith('Incremental'), r
        rest = r[len('Incremental'):]
        self._with_blur = rest.endswith('_with_blur')
        if self._with_blur:
            rest = rest[:-len('_with_blur')]
        self._factor2 = rest.endswith('_factor_2')
        if self._factor2:
            rest = rest[:-len('_factor_2')]
        self._mode = D.PIX_MODES[self._MODES[rest]]
        if self._factor2:
            dec = [self.image_size - self.image_size // 2 ** (i + 1) for i in range(self.num_timesteps)]
        else:
            dec = list(range(self.num_timesteps))
        self._sizes_host = [self.image_size - d for d in dec]      # F.interpolate(size = H - dec_size)
        self._blur_taps = D.gaussian_kernel2d((3, 3), (0.5, 0.5))[None].repeat(self.channels, 1, 1).contiguous()

    def _sizes(self, device):
        key = str(device)
        if key not in self._sizes_cache:
            self._sizes_cache[key] = torch.tensor(self._sizes_host, dtype=torch.int32, device=device)
        return self._sizes_cache[key]

    def transform_func(self, img, dec_size, mode, do_blur=False):
        """The reference's one-step operator with its own signature (RESOL:354-385): [3x3 blur ->] interpolate down to H - dec_size in
        `mode` -> nearest-exact back up [-> 3x3 blur].  `func[i]` of the reference is this with the routine's (dec_size, mode, do_blur)."""
        img = rt.check(img)
        if do_blur:
            taps = self._blur_taps.to(img.device)
            img = D.blur_step(img, taps, 3, 1)
        size = torch.tensor([img.shape[2] - int(dec_size)], dtype=torch.int32, device=img.device)
        img = D.pixelate_chain(img, size, D.PIX_MODES[mode], step_lo=0, step_hi=0)
        if do_blur:
            img = D.blur_step(img, taps, 3, 1)
        return img

    def _step(self, img, i):
        """func[i] with the step's size read from the device-resident table (no host tensor per call)."""
        img = rt.check(img)
        if self._with_blur:
            taps = self._blur_taps.to(img.device)
            img = D.blur_step(img, taps, 3, 1)
        img = D.pixelate_chain(img, self._sizes(img.device), self._mode, step_lo=i, step_hi=i)
        if self._with_blur:
            img = D.blur_step(img, taps, 3, 1)
        return img

    def get_funcs(self):
        return [(lambda img, i=i: self._step(img, i)) for i in range(self.num_timesteps)]

    def _degrade(self, x, nsteps, t=None, img=None):
        if not self._with_blur:
            return D.pixelate_chain(x, self._sizes(x.device), self._mode, t=t, step_lo=0, step_hi=nsteps - 1, img=img)
        assert t is None
        prev = x
        for i in range(nsteps):
            prev = x
            x = self._step(x, i)
        return D.x0_step_down(img, x, prev) if img is not None else x

    # -- sampler graph mode (graphsample.py) ------------------------------------------------------------------------------
    def _sg_why(self):
        if self._with_blur:
            return "the *_with_blur routines run one launch per step from a host step count"
        if self.train_routine != 'Final':
            return "train_routine is not 'Final'"
        return None

    def _sg_step(self, cur, tb):
        x = self.denoise_fn(cur, tb.step)
        if self.sampling_routine == 'default':
            return x, self._degrade(x, 0, t=tb.prev)
        if self.sampling_routine == 'x0_step_down':
            return x, self._degrade(x, 0, t=tb.step, img=cur)
        return x, x

    @torch.no_grad()
    def sample(self, batch_size=16, img=None, t=None, graph=None):
        if t is None:
            t = self.num_timesteps
        img = self._degrade(rt.check(img), t)
        xt, direct_recons = img, None
        sg = self._sg(graph)
        if sg is not None:
            done = sg.reverse('reverse', self._sg_step, img, t, batch_size, why=self._sg_why())
            if done is not None:
                direct_recons, img, t, _ = done
        while t:
            step = _full_step(batch_size, t - 1, img.device)
            x = self.denoise_fn(img, step)
            if self.train_routine == 'Final':
                if direct_recons is None:
                    direct_recons = x
                if self.sampling_routine == 'default':
                    x = self._degrade(x, t - 1)
                elif self.sampling_routine == 'x0_step_down':
                    x = self._degrade(x, t, img=img)
            img = x
            t = t - 1
        return xt, direct_recons, img

    def _reverse_update(self, img, x, times):
        if self.train_routine == 'Final':
            if self.sampling_routine == 'default':
                return self._degrade(x, times - 1)
            if self.sampling_routine == 'x0_step_down':
                return self._degrade(x, times, img=img)
        return x

    @torch.no_grad()
    def gen_sample(self, batch_size=16, img=None, t=None, times=None, noise_level=0, graph=None):
        """No forward process: `times` reverse updates from the given image (RESOL:460-505)."""
        if t is None:
            t = self.num_timesteps
        if times is None:
            times = t
        img = rt.check(img)
        img = img + torch.randn_like(img) * noise_level
        direct_recons = None
        xt = img
        sg = self._sg(graph)
        if sg is not None:
            done = sg.reverse('reverse', self._sg_step, img, times, batch_size, why=self._sg_why())
            if done is not None:
                direct_recons, img, times, _ = done
        while times:
            step = _full_step(batch_size, times - 1, img.device)
            x = self.denoise_fn(img, step)
            if direct_recons is None:
                direct_recons = x
            img = self._reverse_update(img, x, times)
            times = times - 1
        return xt, direct_recons, img

    @torch.no_grad()
    def all_sample(self, batch_size=16, img=None, t=None, times=None, graph=None):
        """Every x0 estimate and every x_t of the reverse process (RESOL:508-556)."""
        if t is None:
            t = self.num_timesteps
        if times is None:
            times = t
        img = self._degrade(rt.check(img), t)
        X_0s, X_ts = [], []
        sg = self._sg(graph)
        if sg is not None:
            done = sg.reverse('all_sample', self._sg_step, img, times, batch_size, put='cur', why=self._sg_why())
            if done is not None:
                _, img, times, (X_0s, X_ts) = done
        while times:
            step = _full_step(batch_size, times - 1, img.device)
            x = self.denoise_fn(img, step)
            X_0s.append(x)
            X_ts.append(img)
            img = self._reverse_update(img, x, times)
            times = times - 1
        return X_0s, X_ts

    @torch.no_grad()
    def forward_and_backward(self, batch_size=16, img=None, t=None, times=None, eval=True, graph=None):
        """The forward trajectory step by step, then every x_t on the way back (RESOL:559-617)."""
        self._sg_eager(graph, "forward_and_backward keeps every step's image: not captured")
        if eval:
            self.denoise_fn.eval()
        if t is None:
            t = self.num_timesteps
        if times is None:
            times = t
        img = rt.check(img)
        Forward = [img]
        for i in range(t):
            img = self._step(img, i)
            Forward.append(img)
        Backward = []
        while times:
            step = _full_step(batch_size, times - 1, img.device)
            x = self.denoise_fn(img, step)
            Backward.append(img)
            img = self._reverse_update(img, x, times)
            times = times - 1
        return Forward, Backward, img

    @torch.no_grad()
    def opt(self, img, t=None):
        if t is None:
            t = self.num_timesteps
        return self._degrade(rt.check(img), t)

    def q_sample(self, x_start, t):
        x_start = rt.check(x_start)
        if not self._with_blur:
            return self._degrade(x_start, 0, t=t.contiguous())
        max_iters = int(torch.max(t))
        x, out = x_start, torch.empty_like(x_start)
        for i in range(max_iters + 1):
            x = self._step(x, i)
            out = torch.where((t == i).view(-1, 1, 1, 1), x, out)
        return out

    def _final_loss(self, x_start, t):
        x_blur = self.q_sample(x_start=x_start, t=t)
        x_recon = self.denoise_fn(x_blur, t)
        return D.loss(x_start, x_recon, self.loss_type)

    @staticmethod
    def _random_mean(x_start):
        """x_start with every (sample, channel) mean replaced by a N(0,1) draw (RESOL:683-691)."""
        new_mean = torch.randn_like(torch.mean(x_start, [2, 3]))
        return x_start - torch.mean(x_start, [2, 3], keepdim=True) + new_mean[:, :, None, None]

    def p_losses(self, x_start, t):
        """RESOL:655-760: 'Final' and its five alternatives."""
        if self.loss_type not in ('l1', 'l2'):
            raise NotImplementedError()
        r = self.train_routine
        if r == 'Final':
            return self._final_loss(x_start, t)
        if r == 'Final_small_noise':
            return self._final_loss(x_start + 0.001 * torch.randn_like(x_start), t)
        if r == 'Final_random_mean':
            return self._final_loss(self._random_mean(x_start), t)
        if r == 'Final_random_mean_and_actual':
            loss1 = self._final_loss(x_start, t)
            return loss1 + self._final_loss(self._random_mean(x_start), t)
        if r == 'Gradient_norm':
            # RESOL:738 calls LA.norm(gradient, dim=(1,2,3)), which torch.linalg.norm rejects, so the routine raises upstream;
            # implemented with its evident intent, the 2-norm over all non-batch dims.
            x_blur = self.q_sample(x_start=x_start, t=t)
            grad_pred = self.denoise_fn(x_blur, t)
            gradient = x_blur - x_start
            norm = gradient.flatten(1).norm(dim=1).view(-1, 1, 1, 1)
            return D.loss(gradient / (norm + 1e-5), grad_pred, self.loss_type)
        if r == 'Step':
            x_blur = self.q_sample(x_start=x_start, t=t)
            # `all_blurs[t - 1, b]` with t = 0 indexes the stack from the END (RESOL:641-646): sample b gets step max(t - 1)
            ts = t - 1
            m = int(ts.max())
            if m < 0:
                raise RuntimeError("stack expects a non-empty TensorList")     # what torch.stack([]) raises upstream
            x_blur_sub = self.q_sample(x_start=x_start, t=torch.where(ts < 0, ts + (m + 1), ts))
            return D.loss(x_blur_sub, self.denoise_fn(x_blur, t), self.loss_type)
        raise UnboundLocalError("local variable 'loss' referenced before assignment")   # unknown routine upstream (RESOL:760)

    def forward(self, x, *args, **kwargs):
        b, c, h, w, device, img_size = *x.shape, x.device, self.image_size
        assert h == img_size and w == img_size, f'height and width of image must be {img_size}'
        t = torch.randint(0, self.num_timesteps, (b,), device=device).long()
        return self.p_losses(x, t, *args, **kwargs)


# ===================================================================================================
# defading (Gaussian-mask inpainting)
# ===================================================================================================
class DefadeDiffusion(TwoPhase, nn.Module):
    def __init__(self, defade_fn, *, image_size, device_of_kernel, channels=3, timesteps=1000, loss_type='l1', kernel_std=0.1,
                 initial_mask=11, fade_routine='Incremental', sampling_routine='default', discrete=False):
        super().__init__()
        self.channels = channels
        self.image_size = image_size
        self.defade_fn = defade_fn
        self.device_of_kernel = device_of_kernel
        self.num_timesteps = int(timesteps)
        self.loss_type = loss_type
        self.kernel_std = kernel_std
        self.initial_mask = initial_mask
        self.fade_routine = fade_routine
        self.fade_kernels = self.get_kernels()
        self.sampling_routine = sampling_routine
        self.discrete = discrete

    def get_fade_kernel(self, dims, std):
        fade_kernel = D.gaussian_kernel2d(dims, std)
        fade_kernel = fade_kernel / torch.max(fade_kernel)
        fade_kernel = torch.ones_like(fade_kernel) - fade_kernel
        return fade_kernel[1:, 1:]

    def get_kernels(self):
        kernels, n = [], self.image_size
        for i in range(self.num_timesteps):
            if self.fade_routine == 'Incremental':
                s = self.kernel_std * (i + self.initial_mask)
                kernels.append(self.get_fade_kernel((n + 1, n + 1), (s, s)))
            elif self.fade_routine == 'Constant':
                kernels.append(self.get_fade_kernel((n + 1, n + 1), (self.kernel_std, self.kernel_std)))
            elif self.fade_routine == 'Random_Incremental':
                s = self.kernel_std * (i + self.initial_mask)
                kernels.append(self.get_fade_kernel((2 * n + 1, 2 * n + 1), (s, s)))
        return torch.stack(kernels)

    def _masks(self, device):
        if self.fade_kernels.device != device:
            self.fade_kernels = self.fade_kernels.to(device)
        return self.fade_kernels.contiguous()

    def _offsets(self, batch_size, device):
        if 'Random' not in self.fade_routine:
            return None, None
        assert self.channels == 3, "the Random_* routines stack exactly three mask channels (DEFADE:514-516)"
        rand_x = torch.randint(0, self.image_size + 1, (batch_size,), device=device).long()
        rand_y = torch.randint(0, self.image_size + 1, (batch_size,), device=device).long()
        return rand_x, rand_y        # rows are cropped at rand_x, columns at rand_y (DEFADE:503-507)

    @torch.no_grad()
    def _sample_impl(self, batch_size, faded, t, times, collect, graph=None):
        faded = rt.check(faded)
        masks = self._masks(faded.device)
        oy, ox = self._offsets(batch_size, faded.device)
        if t is None:
            t = self.num_timesteps
        if times is None:
            times = t
        faded = D.mask_chain(faded, masks, step_lo=0, step_hi=t - 1, off_y=oy, off_x=ox, quantise=self.discrete)
        xt, direct_recons, recon = faded, None, None
        x0_list, xt_list = [], []
        sg = self._sg(graph)
        if sg is not None:
            def step(cur, tb):
                x0 = self.defade_fn(cur, tb.step)
                oy_, ox_ = tb.st.get('oy'), tb.st.get('ox')
                if self.sampling_routine == 'default':
                    return x0, D.mask_chain(x0, masks, t=tb.prev, off_y=oy_, off_x=ox_)
                return x0, D.mask_chain(x0, masks, t=tb.step, img=cur, off_y=oy_, off_x=ox_)
            why = None if self.sampling_routine in ('default', 'x0_step_down') else "unknown sampling_routine: the step is a no-op"
            done = sg.reverse('all_sample' if collect else 'reverse', step, faded, times, batch_size, st={'oy': oy, 'ox': ox},
                              put='next' if collect else None, why=why)
            if done is not None:
                direct_recons, faded, times, lists = done
                recon = faded
                if collect:
                    x0_list, xt_list = lists
        while times:
            step = _full_step(batch_size, times - 1, faded.device)
            recon = self.defade_fn(faded, step)
            x0_list.append(recon)
            if direct_recons is None:
                direct_recons = recon
            if self.sampling_routine == 'default':
                faded = D.mask_chain(recon, masks, step_lo=0, step_hi=times - 2, off_y=oy, off_x=ox)
            elif self.sampling_routine == 'x0_step_down':
                faded = D.mask_chain(recon, masks, step_lo=0, step_hi=times - 1, img=faded, off_y=oy, off_x=ox)
            recon = faded
            xt_list.append(faded)
            times -= 1
        return (x0_list, xt_list) if collect else (xt, direct_recons, recon)

    def sample(self, batch_size=16, faded_recon_sample=None, t=None, graph=None):
        return self._sample_impl(batch_size, faded_recon_sample, t, None, False, graph)

    def all_sample(self, batch_size=16, faded_recon_sample=None, t=None, times=None, graph=None):
        return self._sample_impl(batch_size, faded_recon_sample, t, times, True, graph)

    def q_sample(self, x_start, t):
        x_start = rt.check(x_start)
        oy, ox = self._offsets(x_start.size(0), x_start.device)
        return D.mask_chain(x_start, self._masks(x_start.device), t=t.contiguous(), off_y=oy, off_x=ox, quantise=self.discrete)

    def p_losses(self, x_start, t):
        x_fade = self.q_sample(x_start=x_start, t=t)
        x_recon = self.defade_fn(x_fade, t)
        return D.loss(x_start, x_recon, self.loss_type)

    def forward(self, x, *args, **kwargs):
        b, c, h, w, device, img_size = *x.shape, x.device, self.image_size
        assert h == img_size and w == img_size, f'height and width of image must be {img_size}'
        t = torch.randint(0, self.num_timesteps, (b,), device=device).long()
        self.fade_kernels = self.fade_kernels.to(device)
        return self.p_losses(x, t, *args, **kwargs)
