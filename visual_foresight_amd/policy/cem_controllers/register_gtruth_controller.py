"""CEM controller that re-localises the designated pixels by registering the current frame.

Behavioural restatement of the reference's
``visual_mpc/policy/cem_controllers/register_gtruth_controller.py`` (``Register_Gtruth_Controller``
:10, defaults :28-40, ``register_gtruth`` :54-111, ``act`` :175-195).  That file is mid-refactor in
the reference snapshot - it imports three modules that do not exist and calls a parent method that
was removed - so it documents intent rather than runnable behaviour; this class implements that
intent on top of ``PixelCostController``:

* ``ndesig = ntask * len(register_gtruth)`` designated pixels per camera: every task is tracked
  once per registration target ('start' frame and/or 'goal' image), ``:25``;
* at the first CEM iteration of every planning call the plug-in warper registers the current
  frame to the start frame / goal image, the tracked pixels replace the designated pixels and the
  warp errors give the trade-off weights ``plan_stat['tradeoff']``, ``:46-50,88-94``;
* goal pixels are tiled across registrations, ``:179-181``.

The reference stores the trade-off but its parent scores with a plain mean over tasks
(``pixel_cost_controller.py:153``); ``trade_off_reg=True`` (the reference's commented-out
hyper-parameter, ``:32``) applies the weights, ``False`` keeps the plain mean.

With a predictor that offers ``register()`` (``HipVPredEvaluation``) the arithmetic of
``get_warp_err`` - bilinear warp of the current frame by the registration network's flow field,
window median of the warp points, photometric warp error - runs on the GPU (``vf_register``,
``include/vf_hip.h``) and the trade-off weights are applied inside the fused score kernel; the
warper only has to supply the flow field.  With ``HipRegistrationNet``
(``video_prediction/registration_net.py``) as the warper the flow fields of all registrations come
from one ``flow_device`` call on the predictor's device and never visit the host.  Any other
predictor takes the NumPy path of ``registration.py`` on the warper's own ``(warped, flow, warp_pts)``.

Two resolutions (``model_image_height`` / ``model_image_width`` in ``ag_params``, the reference's ``:44-51,121-128,172,
183,191`` - its one shipped registration experiment runs a 96 x 128 agent on a 48 x 64 predictor): ``desig_pix`` /
``goal_pix`` arrive in MODEL coordinates; registration runs at the CAMERA's resolution - camera-size current frame, start
frame and goal image, a warper built at that size, the medium-resolution pixel tables ``(pix * image_height /
img_height).astype(int)``, the window ``5 if image_height >= 96 else 2`` clipped with the camera's dimensions
(``vf_register_hw``, or ``registration.get_warp_err`` on the NumPy path) - and the tracked pixels are multiplied by
``img_height / image_height`` before they become the designated pixels of the rollout, which runs at the model's size.
"""
import numpy as np

from .pixel_cost_controller import PixelCostController
from .registration import get_warp_err, medium_res_pixels, model_res_pixels, tradeoff_weights


class RegisterGtruthController(PixelCostController):
    def __init__(self, ag_params, policyparams, gpu_id, ngpu):
        super(RegisterGtruthController, self).__init__(ag_params, policyparams, gpu_id, ngpu)
        nreg = len(self._hp.register_gtruth)
        if nreg == 0 or self._n_desig % nreg:
            raise ValueError('designated_pixel_count must be a multiple of len(register_gtruth)')
        self.ntask = self._n_desig // nreg
        self.goal_image_warper = self._hp.registration_warper
        self.reg_tradeoff = np.ones([self._n_cam, self._n_desig]) / self._n_cam / self._n_desig
        self.start_image = None
        # the agent's (camera's) height; self._img_height is the model's (pixel_cost_controller.model_image_size)
        self._image_height = ag_params['image_height']
        self._two_res = self._image_height != self._img_height

    def _default_hparams(self):
        params = super(RegisterGtruthController, self)._default_hparams()
        params.add_hparam('register_gtruth', ['start', 'goal'])
        params.add_hparam('register_region', False)
        params.add_hparam('trade_off_reg', False)
        params.add_hparam('registration_warper', None)    # callable, see registration.py
        params.add_hparam('registration_on_device', True)  # use predictor.register() when it exists
        return params

    # ------------------------------------------------------------------ registration
    def register_gtruth(self, start_image, current_image):
        """-> (tracked desig pixels [ncam, ndesig, 2], trade-off [ncam, ndesig]) for this frame."""
        # (registration runs where predictor.register runs: on the first lane's device of an in-process multi-GPU predictor)
        if self.goal_image_warper is None:
            raise ValueError("RegisterGtruthController needs the 'registration_warper' hyper-parameter")
        regs = self._hp.register_gtruth
        H = start_image.shape[1]
        # registration runs at the agent's resolution, on the medium-resolution tables when the model's differs (:121-128)
        pix_t0, goal_pix = (self.desig_pix_t0_med, self.goal_pix_med) if self._two_res else (self.desig_pix_t0, self.goal_pix_sel)
        if hasattr(self.predictor, 'register') and self._hp.registration_on_device:
            region = (5 if H >= 96 else 2) if self._hp.register_region else 0
            per_reg = []
            targets = [(ref, pix, clip) for name, ref, pix, clip in
                       (('start', start_image, pix_t0, 1), ('goal', self.goal_image, goal_pix, 0))
                       if name in regs]
            if hasattr(self.goal_image_warper, 'flow_device'):
                # a registration network on the device: one call for all registrations, the flow stays on the card
                net, pred_dev = self.goal_image_warper, getattr(self.predictor, 'device', None)
                if pred_dev is not None and net.device != pred_dev:
                    raise ValueError('the registration net lives on %s, the predictor registers on %s (use clone_to)'
                                     % (net.device, pred_dev))
                # every image is uploaded once: the net and predictor.register both read the device copies
                import torch
                d_cur = torch.from_numpy(np.ascontiguousarray(current_image, dtype=np.float32)).to(net.device)
                d_refs = torch.from_numpy(np.stack([np.asarray(ref, dtype=np.float32) for ref, _, _ in targets])).to(net.device)
                flows = net.flow_device(d_cur.expand_as(d_refs), d_refs)
                for i, (_, pix, clip) in enumerate(targets):
                    per_reg.append(self.predictor.register(d_cur, d_refs[i], flows[i], pix, region=region, clip_sub=clip))
            else:
                for ref, pix, clip in targets:
                    _, flow, _ = self.goal_image_warper(current_image, ref)
                    per_reg.append(self.predictor.register(current_image, ref, flow, pix, region=region, clip_sub=clip))
            desig = [np.stack([d[icam] for d, _ in per_reg], axis=1) for icam in range(self._n_cam)]   # [ntask, nreg, 2]
            errs = [np.stack([e[icam] for _, e in per_reg], axis=1) for icam in range(self._n_cam)]    # [ntask, nreg]
            if self._two_res:       # camera coordinates -> the model's (:172)
                desig = [model_res_pixels(d, self._img_height, self._image_height) for d in desig]
        else:
            warped_start = start_pts = warped_goal = goal_pts = None
            if 'start' in regs:
                warped_start, _, start_pts = self.goal_image_warper(current_image, start_image)
            if 'goal' in regs:
                warped_goal, _, goal_pts = self.goal_image_warper(current_image, self.goal_image)
            errs, desig = [], []
            for icam in range(self._n_cam):
                e, d = get_warp_err(icam, pix_t0[icam], goal_pix[icam], start_image,
                                    self.goal_image, start_pts, goal_pts, warped_start, warped_goal,
                                    register_gtruth=regs, register_region=self._hp.register_region,
                                    pred_height=self._img_height if self._two_res else None)
                errs.append(e)
                desig.append(d)
        warperrs = np.stack(errs, 0)                                    # [ncam, ntask, nreg]
        tradeoff = tradeoff_weights(warperrs).reshape(self._n_cam, self._n_desig)
        self.plan_stat['tradeoff'] = tradeoff
        self.plan_stat['warperrs'] = warperrs.reshape(self._n_cam, self._n_desig)
        return np.stack(desig, 0).reshape(self._n_cam, self._n_desig, 2), tradeoff

    def evaluate_rollouts(self, actions, cem_itr):
        self._register_at_first_iteration(cem_itr)
        return super(RegisterGtruthController, self).evaluate_rollouts(actions, cem_itr)

    def _register_at_first_iteration(self, cem_itr):
        if self._hp.register_gtruth and cem_itr == 0:
            current = self._images[-1].astype(np.float32) / 255.
            self._desig_pix, self.reg_tradeoff = self.register_gtruth(self.start_image, current)

    # ------------------------------------------------------------------ device-resident CEM
    def _device_cem_plan(self):
        """The parent's refusals against this class's own ``evaluate_rollouts``, and registration through
        ``predictor.register`` (``registration_on_device``): the NumPy path of ``registration.py`` plans on the host."""
        if not (hasattr(self.predictor, 'register') and self._hp.registration_on_device):
            return None
        return self._pixel_cost_device_plan(RegisterGtruthController.evaluate_rollouts)

    def _score_device_candidates(self, candidates, itr):
        """Register before the first rollout - ``register()`` downloads the tracked pixels and warp errors, the one
        synchronisation of the call besides its download - then score as the parent does (the trade-off weights reach the
        rollout through ``_task_weights``)."""
        self._register_at_first_iteration(itr)
        return super(RegisterGtruthController, self)._score_device_candidates(candidates, itr)

    def _task_weights(self):
        return self.reg_tradeoff if self._hp.trade_off_reg else None

    def act(self, goal_image=None, t=None, i_tr=None, desig_pix=None, goal_pix=None, images=None, state=None,
            verbose_worker=None):
        """``goal_image`` [.., ncam, H, W, 3] float in [0,1] (the last entry is used, ``:186``), at the agent's size;
        ``desig_pix`` / ``goal_pix`` in the model's coordinates."""
        nreg = len(self._hp.register_gtruth)
        self.goal_pix_sel = np.array(goal_pix).reshape((self._n_cam, self.ntask, 2))
        goal_tiled = np.tile(self.goal_pix_sel[:, :, None, :], [1, 1, nreg, 1])
        self.goal_pix_med = medium_res_pixels(self.goal_pix_sel, self._image_height, self._img_height)     # (:183)
        self.goal_image = np.asarray(goal_image)[-1]
        if t == 0:
            self.desig_pix_t0 = np.array(desig_pix).reshape((self._n_cam, self.ntask, 2))
            self.desig_pix_t0_med = medium_res_pixels(self.desig_pix_t0, self._image_height, self._img_height)     # (:191)
            self.start_image = np.asarray(images)[0].astype(np.float32) / 255.
        desig_tiled = np.tile(self.desig_pix_t0[:, :, None, :], [1, 1, nreg, 1])
        return super(RegisterGtruthController, self).act(
            t=t, i_tr=i_tr, desig_pix=desig_tiled.reshape(self._n_cam, self._n_desig, 2),
            goal_pix=goal_tiled.reshape(self._n_cam, self._n_desig, 2), images=images, state=state,
            verbose_worker=verbose_worker)
