"""The six `GaussianDiffusion` classes of the cold-diffusion packages, on the HIP degradation kernels.

Constructor arguments, attribute names, method names, return values and `state_dict` layout follow
  deblurring  : deblurring_diffusion_pytorch.py:311-981
  denoising   : denoising_diffusion_pytorch.py:310-542
  demixing    : demixing_diffusion_pytorch.py:309-502
  defading generation : defading_diffusion_pytorch.py:309-568
  resolution  : resolution_diffusion_pytorch.py:325-767
  defading    : defading_diffusion_gaussian.py:298-554
What differs is the execution: q_sample and every Alg.1/Alg.2 sampler step is ONE fused kernel
launch (the whole step chain runs with the image plane resident in LDS) instead of O(T) convs, a
torch.stack of T images and B python-level gathers, and nothing synchronises with the host
(the reference's `torch.max(t)` -> `range()` does).

What the six share is written once.  The reverse loop of every sampler is `SampleGraphMixin._walk` (graphsample.py): a sampler
method does its forward process, hands the walk its core's step rule and, where it keeps per-step images, a collector, and packs
the return value.  Each core has ONE `_update`, the `sampling_routine` / `train_routine` dispatch of a reverse step, with the
ordinary form (host step count, `cdf_noise_step` / `cdf_blend_step`) and the captured form (the step table's rows, the `_dev`
entry points) side by side.  `forward` and the 'Final' loss are `TwoPhase`'s (`TwoImage` for the cores with a second image).
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

    def _final_loss(self, x_start, t, *x_end):
        """The 'Final' training routine: the network's estimate from q_sample(x_start, [x_end,] t) against x_start."""
        return self.loss_prepared((x_start, t, self.q_sample(x_start, *x_end, t)))

    def p_losses(self, x_start, t):
        if self.fusable():
            return self._final_loss(x_start, t)
        raise NotImplementedError()

    def forward(self, x, *args, **kwargs):
        return self.p_losses(x, self._draw_t(x), *args, **kwargs)


class TwoImage(TwoPhase):
    """TwoPhase for the cores whose forward process blends x1 into a second image: `forward(x1, x2)`, `p_losses(x_start, x_end, t)`."""

    def p_losses(self, x_start, x_end, t):
        if self.fusable():
            return self._final_loss(x_start, t, x_end)
        raise NotImplementedError()

    def forward(self, x1, x2, *args, **kwargs):
        return self.p_losses(x1, x2, self._draw_t(x1), *args, **kwargs)


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

    def _fused(self, H, W):
        """Is the blur chain ONE LDS-resident launch at this plane size (else: one launch per step, from host step counts)."""
        return self._uniform() and D.blur_fits_lds(H, W, self.gaussian_kernels[0].weight.shape[-1])

    def _degrade(self, x, nsteps, t=None, img=None, quantise=False, collapse=True):
        """D(x, nsteps): kernels 0..nsteps-1 (or 0..t[b] per sample; with img: the Alg.2 combination), the discrete mean-collapse
        included unless `collapse=False` drops it."""
        _, _, H, W = x.shape
        collapse = self.num_timesteps - 1 if self.discrete and collapse else -1
        if self._fused(H, W):
            k = self.gaussian_kernels[0].weight.shape[-1]
            return D.blur_chain(x, self._taps(x.device), k, self._pad_mode(), t=t, step_lo=0, step_hi=nsteps - 1, img=img,
                                collapse_step=collapse, quantise=quantise, taps1d=self._taps1d(x.device))
        assert t is None and not quantise, "per-sample t needs the LDS-resident path"
        prev = x
        for i in range(nsteps):
            prev = x
            x = self._apply_one(i, x)
            if i == collapse:
                x = D.plane_mean_(x)
        return D.x0_step_down(img, x, prev) if img is not None else x

    def _collapse(self, img):
        return D.plane_mean_(img.clone()) if self.discrete else img

    # -- samplers (DEBLUR:393-689) --------------------------------------------------------------------
    def _forward_process(self, img, t):
        if self.blur_routine == 'Individual_Incremental':
            return self._apply_one(t - 1, img)
        return self._degrade(img, t, collapse=False)         # the forward pass never mean-collapses inside the loop

    def _update(self, img, x, t, tb=None, routine=None):
        """The reverse step's rule, x_t = img and the estimate x -> x_{t-1}, under `routine` (default: the core's own; only
        forward_and_backward_2 names one).  Ordinary form: `t` is the host step count; captured form: the step table `tb`."""
        if routine is None:
            if self.train_routine != 'Final':
                return x
            routine = self.sampling_routine
            if routine == 'default' and not self._uniform():
                return self._apply_one(t - 2, x)             # (one kernel per step, picked by a host index: never captured)
        if routine == 'default':                             # D(x, t - 1); the Alg.1 chain has no collapse (DEBLUR:432-434)
            if tb is not None:
                return self._degrade(x, 0, t=tb.prev, collapse=False)      # row -1 is the identity
            return self._degrade(x, t - 1, collapse=False)
        if routine == 'x0_step_down':                        # img - D(x, t) + D(x, t - 1)
            return self._degrade(x, 0, t=tb.step, img=img) if tb is not None else self._degrade(x, t, img=img)
        return x

    def _update_xt_quirk(self, img, x, t, tb=None, any_routine=False):
        """_update as all_sample and forward_and_backward apply it: under Individual_Incremental the reference blurs x_t instead of
        the estimate -- all_sample whatever the sampling routine (DEBLUR:645-647), forward_and_backward under the two it knows
        (DEBLUR:731-733, 744-746) -- and leaves the estimate alone at the last step."""
        if self._uniform() or self.train_routine != 'Final':
            return self._update(img, x, t, tb)
        if t - 2 >= 0 and (any_routine or self.sampling_routine in ('default', 'x0_step_down')):
            return self._apply_one(t - 2, img)
        return x

    def _sg_why(self):
        """Why the reverse step of this core cannot run with every `t` read from the step table (graphsample.py), or None."""
        if not self._uniform():
            return "blur_routine='Individual_Incremental' applies one kernel per step, picked by a host index"
        if not self._fused(self.image_size, self.image_size):
            return "the plane is past the LDS cap: the per-step blur fallback takes host step counts"
        if self.train_routine != 'Final':
            return "train_routine is not 'Final'"
        return None

    @torch.no_grad()
    def _sample_impl(self, batch_size, img, t, noise_level, graph=None):
        self.denoise_fn.eval()
        if t is None:
            t = self.num_timesteps
        img = self._forward_process(rt.check(img), t)
        img = self._collapse(img)
        if noise_level is not None:
            img = img + torch.randn_like(img) * noise_level
        return (img,) + self._reverse_loop(batch_size, img, t, graph)

    def _reverse_loop(self, batch_size, img, t, graph=None):
        direct_recons, img = self._walk(img, t, batch_size, self._update, graph=graph, variant='reverse', why=self._sg_why)
        return (direct_recons if self.train_routine == 'Final' else None), img

    def sample(self, batch_size=16, img=None, t=None, graph=None):
        out = self._sample_impl(batch_size, img, t, None, graph)
        self.denoise_fn.train()
        return out

    def gen_sample(self, batch_size=16, img=None, t=None, noise_level=0, graph=None):
        return self._sample_impl(batch_size, img, t, noise_level, graph)

    gen_sample_2 = gen_sample

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
        if self.blur_routine == 'Individual_Incremental':
            img = self._apply_one(t - 1, img)
        else:
            Forward += self._trajectory(img, 0, t)
            img = Forward[-1]
        Backward = []
        if self.discrete:
            img = self._collapse(img)
            img = img + torch.randn_like(img) * noise_level
        _, img = self._walk(img, times, batch_size, self._update_xt_quirk, collect=lambda x, x_t: Backward.append(x_t))
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
        backs, ends = [], []
        for routine in ('default', 'x0_step_down'):
            backs.append([])
            ends.append(self._walk(img, T, batch_size, lambda x_t, x, t, tb, r=routine: self._update(x_t, x, t, tb, r),
                                   collect=lambda x, x_t: backs[-1].append(x_t))[1])
        return Forward, backs[0], backs[1], ends[0], ends[1]

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
        if t > start and self._fused(*img.shape[2:]):
            img = D.blur_chain(img, self._taps(img.device), self.gaussian_kernels[0].weight.shape[-1], self._pad_mode(), step_lo=start,
                               step_hi=t - 1, taps1d=self._taps1d(img.device))
        else:
            for i in range(start, t):
                img = self._apply_one(i, img)
        img = self._collapse(img)
        return (img,) + self._reverse_loop(batch_size, img, t, graph)

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
        _, img = self._walk(img, times, batch_size, lambda x_t, x, t, tb: self._update_xt_quirk(x_t, x, t, tb, any_routine=True),
                            collect=lambda x, x_t: (X_0s.append(x), X_ts.append(x_t)), graph=graph, variant='all_sample', put='cur',
                            why=self._sg_why)
        if self.discrete:
            img = img - noise
        X_0s.append(img)
        self.denoise_fn.train()
        return X_0s, X_ts

    # -- training (DEBLUR:927-981): p_losses and forward are TwoPhase's ------------------------------------------
    def q_sample(self, x_start, t):
        x_start = rt.check(x_start)
        if self._fused(*x_start.shape[2:]):
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

    # -- forward() in two phases, for the Trainer's degradation prefetch: the blur chain of micro-batch i+1 (up to T sequential
    # steps on B*C planes: 96 of 256 CUs at B = 32) does not depend on the network and runs on a side stream under the
    # forward / backward of micro-batch i.  prepare() + loss_prepared() == forward(): same draws, same kernels.
    def can_prepare_async(self):
        """True when q_sample is ONE sync-free launch (uniform kernel size, plane fits the LDS): only then does a side-stream
        prefetch overlap with anything -- the per-step fallback reads max(t) on the host and would block the launching thread."""
        return self._fused(self.image_size, self.image_size)

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


class DenoiseDiffusion(TwoImage, nn.Module):
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

    def _update(self, img, x1_bar, t, tb, noise, est_noise):
        """x_t = img and the estimate x1_bar -> x_{t-1}, with the second image estimated from x_t (`est_noise`) or held fixed (`noise`).
        Ordinary form: `t` is the host step count; captured form: the step table `tb`, whose `st` holds the fixed image."""
        ca, cb = self._tables()
        if tb is not None:
            return D.noise_step_dev(img, x1_bar, tb.st.get('noise'), ca, cb, tb.step, est_noise)
        return D.noise_step(img, x1_bar, noise, ca, cb, t, est_noise)

    @torch.no_grad()
    def _reverse(self, batch_size, img, t, est_noise, noise, graph=None, collect=None):
        return self._walk(img, t, batch_size, lambda x_t, x, t, tb: self._update(x_t, x, t, tb, noise, est_noise), collect=collect,
                          graph=graph, variant=('reverse', est_noise), st={'noise': noise})

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
    def _forward_and_backward(self, batch_size, img, x2, t, graph):
        """`img` mixed step by step into ONE second image (`x2`; None: a Gaussian draw), then back with that image held fixed."""
        self._sg_eager(graph, "forward_and_backward keeps every step's image: not captured")
        self.denoise_fn.eval()
        t = self.num_timesteps if t is None else t
        ca, cb = self._tables()
        img = rt.check(img)
        noise = torch.randn_like(img) if x2 is None else rt.check(x2)
        Forward = [img]
        for i in range(t):
            n_img = D.noise_qsample(img, noise, ca, cb, _full_step(batch_size, i, img.device))
            Forward.append(n_img)
        Backward = []
        _, img = self._reverse(batch_size, n_img, t, False, noise, graph=False, collect=lambda x1_bar, x_t: Backward.append(x_t))
        return Forward, Backward, img

    def forward_and_backward(self, batch_size=16, img=None, t=None, times=None, eval=True, graph=None):
        """Noising trajectory with ONE noise draw, then the fixed-noise way back (DENOISE:438-479)."""
        return self._forward_and_backward(batch_size, img, None, t, graph)

    @torch.no_grad()
    def all_sample(self, batch_size=16, img=None, t=None, times=None, eval=True, graph=None):
        self._sg_eager(graph, "all_sample moves every step to the host, as upstream does")
        if eval:
            self.denoise_fn.eval()
        t = self.num_timesteps if t is None else t
        X1_0s, X2_0s, X_ts = [], [], []

        def to_host(x1_bar, x_t):
            step = _full_step(batch_size, t - 1 - len(X_ts), x_t.device)
            x2_bar = self.get_x2_bar_from_xt(x1_bar, x_t, step)
            X1_0s.append(x1_bar.detach().cpu())
            X2_0s.append(x2_bar.detach().cpu())
            X_ts.append(x_t.detach().cpu())

        self._reverse(batch_size, img, t, True, None, graph=False, collect=to_host)
        return X1_0s, X2_0s, X_ts


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

    def forward_and_backward(self, batch_size=16, img1=None, img2=None, t=None, times=None, eval=True, graph=None):
        """img1 mixed step by step into img2, then back with img2 held fixed (DEMIX:416-458)."""
        return self._forward_and_backward(batch_size, img1, img2, t, graph)

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


class DefadeGenDiffusion(TwoImage, nn.Module):
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

    def _update(self, img, x1_bar, t, tb, x2):
        """x_t = img and the estimate x1_bar -> x_{t-1} with the second image x2 held fixed.  Ordinary form: `t` is the host step
        count; captured form: the step table `tb`, whose `st` holds x2."""
        if tb is not None:
            return D.blend_step_dev(img, x1_bar, tb.st['x2'], self.alphas, self.one_minus_alphas, tb.step)
        return D.blend_step(img, x1_bar, x2, self.alphas, self.one_minus_alphas, t)

    @torch.no_grad()
    def _reverse(self, batch_size, img, t, x2, collect=None, graph=None):
        return self._walk(img, t, batch_size, lambda x_t, x, t, tb: self._update(x_t, x, t, tb, x2), collect=collect, graph=graph,
                          variant='reverse', st={'x2': x2},
                          why="every step's images are collected on the way: not captured" if collect is not None else None)

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

    def _update(self, img, x, t, tb=None):
        """The reverse step's rule, x_t = img and the estimate x -> x_{t-1}.  Ordinary form: `t` is the host step count; captured
        form: the step table `tb`."""
        if self.train_routine != 'Final':
            return x
        if self.sampling_routine == 'default':
            return self._degrade(x, 0, t=tb.prev) if tb is not None else self._degrade(x, t - 1)
        if self.sampling_routine == 'x0_step_down':
            return self._degrade(x, 0, t=tb.step, img=img) if tb is not None else self._degrade(x, t, img=img)
        return x

    def _reverse(self, batch_size, img, n, graph, collect=None):
        """`n` reverse steps from x_t = img (the samplers here do not call eval(), as upstream does not)."""
        return self._walk(img, n, batch_size, self._update, collect=collect, graph=graph, variant='all_sample' if collect else 'reverse',
                          put='cur' if collect else None, why=self._sg_why)

    @torch.no_grad()
    def sample(self, batch_size=16, img=None, t=None, graph=None):
        if t is None:
            t = self.num_timesteps
        xt = self._degrade(rt.check(img), t)
        direct_recons, img = self._reverse(batch_size, xt, t, graph)
        return xt, (direct_recons if self.train_routine == 'Final' else None), img

    @torch.no_grad()
    def gen_sample(self, batch_size=16, img=None, t=None, times=None, noise_level=0, graph=None):
        """No forward process: `times` reverse updates from the given image; `direct_recons` is set whatever train_routine is
        (RESOL:460-505)."""
        if t is None:
            t = self.num_timesteps
        if times is None:
            times = t
        img = rt.check(img)
        xt = img + torch.randn_like(img) * noise_level
        return (xt,) + self._reverse(batch_size, xt, times, graph)

    @torch.no_grad()
    def all_sample(self, batch_size=16, img=None, t=None, times=None, graph=None):
        """Every x0 estimate and every x_t of the reverse process (RESOL:508-556)."""
        if t is None:
            t = self.num_timesteps
        if times is None:
            times = t
        img = self._degrade(rt.check(img), t)
        X_0s, X_ts = [], []
        self._reverse(batch_size, img, times, graph, collect=lambda x, x_t: (X_0s.append(x), X_ts.append(x_t)))
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
        _, img = self._walk(img, times, batch_size, self._update, collect=lambda x, x_t: Backward.append(x_t))
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
        return get_fade_kernel(dims, std)

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

    def _update(self, img, x0, t, tb, masks, oy, ox):
        """The reverse step's rule, x_t = img and the estimate x0 -> x_{t-1}.  Ordinary form: `t` is the host step count; captured
        form: the step table `tb`, whose `st` holds the call's crop offsets."""
        if tb is not None:
            oy, ox = tb.st.get('oy'), tb.st.get('ox')
        if self.sampling_routine == 'default':
            if tb is not None:
                return D.mask_chain(x0, masks, t=tb.prev, off_y=oy, off_x=ox)
            return D.mask_chain(x0, masks, step_lo=0, step_hi=t - 2, off_y=oy, off_x=ox)
        if self.sampling_routine == 'x0_step_down':
            if tb is not None:
                return D.mask_chain(x0, masks, t=tb.step, img=img, off_y=oy, off_x=ox)
            return D.mask_chain(x0, masks, step_lo=0, step_hi=t - 1, img=img, off_y=oy, off_x=ox)
        return img                                                   # an unknown routine leaves x_t where it is (never captured)

    @torch.no_grad()
    def _sample_impl(self, batch_size, faded, t, times, collect, graph=None):
        """(the samplers here do not call eval(), as upstream does not; all_sample collects the NEXT x_t of every step)"""
        faded = rt.check(faded)
        masks = self._masks(faded.device)
        oy, ox = self._offsets(batch_size, faded.device)
        if t is None:
            t = self.num_timesteps
        if times is None:
            times = t
        faded = D.mask_chain(faded, masks, step_lo=0, step_hi=t - 1, off_y=oy, off_x=ox, quantise=self.discrete)
        x0_list, xt_list = [], []
        why = None if self.sampling_routine in ('default', 'x0_step_down') else "unknown sampling_routine: the step is a no-op"
        direct_recons, recon = self._walk(faded, times, batch_size, lambda x_t, x0, t, tb: self._update(x_t, x0, t, tb, masks, oy, ox),
                                          collect=(lambda x0, nxt: (x0_list.append(x0), xt_list.append(nxt))) if collect else None,
                                          graph=graph, variant='all_sample' if collect else 'reverse', st={'oy': oy, 'ox': ox},
                                          put='next' if collect else None, why=why)
        return (x0_list, xt_list) if collect else (faded, direct_recons, recon if times else None)

    def sample(self, batch_size=16, faded_recon_sample=None, t=None, graph=None):
        return self._sample_impl(batch_size, faded_recon_sample, t, None, False, graph)

    def all_sample(self, batch_size=16, faded_recon_sample=None, t=None, times=None, graph=None):
        return self._sample_impl(batch_size, faded_recon_sample, t, times, True, graph)

    def q_sample(self, x_start, t):
        x_start = rt.check(x_start)
        oy, ox = self._offsets(x_start.size(0), x_start.device)
        return D.mask_chain(x_start, self._masks(x_start.device), t=t.contiguous(), off_y=oy, off_x=ox, quantise=self.discrete)

    def forward(self, x, *args, **kwargs):
        self._masks(x.device)                                        # (DEFADE's forward moves the masks to the batch's device)
        return super().forward(x, *args, **kwargs)
