"""Config surface - attribute-compatible with reference config.py:15-139 (same tree, same
defaults, same add_g_criterion/remove_g_criterion/get_all_params), plus DIST.* / KERNEL.* knobs.

Differences, all additive:
  * criterion objects default to the HIP-path modules of srganst.loss (same call protocol
    ``criterion(sr, gt) -> 0-dim``); 'Adversarial' keeps its special (D(sr), real_label) call;
  * class-level dicts are copied per instance (the reference shares them between instances,
    config.py:19,33,45,57 - an accident, not an interface).
"""
from __future__ import annotations

import os

import copy

import torch


class dotdict(dict):
    """dot.notation access to dictionary attributes (reference config.py:3-13)."""
    __getattr__ = dict.__getitem__
    __setattr__ = dict.__setitem__
    __delattr__ = dict.__delitem__
    __dir__ = dict.keys
    __repr__ = dict.__repr__


class Config:
    def __init__(self):
        from . import loss as L

        self.DEVICE = "cuda:0" if torch.cuda.is_available() else "cpu"

        self.EXP = dotdict()
        self.EXP.USER = "s204163"
        self.EXP.NAME = "experiment-name"
        self.EXP.START_EPOCH = 0
        self.EXP.N_EPOCHS = 40
        self.EXP.LABEL_SMOOTHING = 0.1
        # Resume (checkpoint.py): a path to a training-state file, or "auto" = results/{NAME}/state_last.pth when it exists, else a
        # fresh start.  The file restores weights, Adam moments and step counters, the LR schedule, the averaged generator, the
        # best validation values and the RNG streams, and START_EPOCH is taken from it.  "" = off
        self.EXP.RESUME = ""
        # the drivers write results/{NAME}/state_last.pth after every epoch (tens of MB for the full model: G, D and their
        # moments).  False: the files written are exactly g_* / d_* as before
        self.EXP.SAVE_STATE = True

        self.LOG_TRAIN_PERIOD = 100
        self.LOG_VALIDATION_PERIOD = 1
        self.D_CHECKPOINT_INTERVAL = 100
        self.G_CHECKPOINT_INTERVAL = 100

        self.DATA = dotdict()
        self.DATA.TRAIN_GT_IMAGES_DIR = f"/work3/{self.EXP.USER}/data/train"
        self.DATA.TEST_SET = "Set5"
        self.DATA.TEST_GT_IMAGES_DIR = f"/work3/{self.EXP.USER}/data/{self.DATA.TEST_SET}/GTmod12"
        self.DATA.TEST_LR_IMAGES_DIR = f"/work3/{self.EXP.USER}/data/{self.DATA.TEST_SET}/LRbicx4"
        self.DATA.TEST_SR_IMAGES_DIR = "results/_test"
        self.DATA.SEED = 0
        self.DATA.UPSCALE_FACTOR = 4
        self.DATA.BATCH_SIZE = 16
        self.DATA.GT_IMAGE_SIZE = 96
        # True: the train()/warmup() drivers decode the training set ONCE into device memory (uint8) and build every batch with one
        # HIP launch (device_data.py: gather + LR synthesis, sst_gather_batch) instead of the host DataLoader; needs the whole HR
        # set in device memory on every rank and crops of one size on the 1/255 grid.  KERNEL.LR_ON_DEVICE does not apply to it
        self.DATA.ON_DEVICE = False
        # True: validation stays on the device - the test pairs are copied to it once (device_data.DeviceTestSet), PSNR / SSIM come
        # from one HIP kernel per image (metrics.py: sst_image_metrics, the host path's numbers up to fp64 summation order) and all
        # results cross to the host in one copy after the loop.  Images must be at least 11 px on each side.  (Beside
        # DATA.ON_DEVICE, not under KERNEL: KERNEL holds the training engine's schedule switches, a set the tests pin exactly)
        self.DATA.VALIDATE_ON_DEVICE = False
        # True: validation also reports the structure-tensor distance of every test image (st.st_distance: the per-image mean of the
        # distance the ``ST`` criterion integrates, with that criterion's sigma / rho / normalize when one is configured, else its
        # defaults): _metrics.txt and the printed line gain an ``ST:`` column, the drivers log Test/ST.  Checkpoint selection is
        # unchanged.  Works with either validation path; on the device path the values cross to the host once, after the loop
        self.DATA.VALIDATE_ST = False
        # True: validation also reports the LR consistency of every test image (metrics.lr_consistency: the output, clamped and
        # downscaled again by the kernel that made the LR input, against the loader's LR image) as an ``LR-PSNR:`` column of
        # _metrics.txt and the printed line, after ``ST:`` when both are on; the drivers log Test/LR-PSNR.  Either validation path
        self.DATA.VALIDATE_LR = False
        # T > 0: validation runs the generator tiled (upscale.Upscaler: windows of T LR pixels with the exact halo, so the whole-image
        # forward's result) - test images of any size, beyond what one whole-image forward takes.  0: whole-image forwards
        self.DATA.VALIDATE_TILE = 0

        # True: the drivers keep the WHOLE training images of TRAIN_ORIGINAL_IMAGES_DIR (any sizes, e.g. DIV2K as distributed) in
        # device memory and one HIP launch per batch cuts, transforms, converts and downscales the samples (device_data.py:
        # DeviceImageArena / DeviceCropLoader, sst_gather_crops).  No crops need to be cut beforehand: an epoch walks the tiles
        # data-prep/prepare_dataset.py would have written (GT_IMAGE_SIZE squares every CROP_STEP pixels), shuffled.  Takes the place of
        # ON_DEVICE when both are set
        self.DATA.ON_DEVICE_WHOLE_IMAGES = False
        self.DATA.TRAIN_ORIGINAL_IMAGES_DIR = f"/work3/{self.EXP.USER}/data/original"
        self.DATA.CROP_STEP = 96
        # with ON_DEVICE_WHOLE_IMAGES only: each sample's window at a uniform position of its image instead of on the tile grid /
        # one of the eight flips and transpositions per sample; drawn per epoch from a private generator seeded by (SEED, epoch)
        self.DATA.RANDOM_CROP = False
        self.DATA.AUGMENT = False
        # with ON_DEVICE_WHOLE_IMAGES only: the classical blind-SR degradation lr = quantise(clamp(bicubic(gt * k) + n)) instead of
        # lr = bicubic(gt), made per sample in the same gather launch (device_data.Degradation, sst_gather_crops_degraded): k an
        # anisotropic Gaussian on a KSIZE x KSIZE window (odd, 3..21) with standard deviations uniform in BLUR_SIGMA (equal when
        # ANISO is off) at a uniform angle, applied with probability BLUR_PROB; n Gaussian noise with a standard deviation uniform
        # in NOISE_SIGMA (0..255 units), applied with probability NOISE_PROB.  Drawn per epoch and tile from a second private
        # generator seeded by (SEED, epoch); gt is untouched
        self.DATA.DEGRADE = False
        self.DATA.DEGRADE_BLUR_SIGMA = (0.2, 4.0)
        self.DATA.DEGRADE_BLUR_ANISO = True
        self.DATA.DEGRADE_BLUR_PROB = 1.0
        self.DATA.DEGRADE_BLUR_KSIZE = 21
        self.DATA.DEGRADE_NOISE_SIGMA = (0.0, 25.0)
        self.DATA.DEGRADE_NOISE_PROB = 1.0
        # with DEGRADE: with probability JPEG_PROB a sample's degraded LR also goes through a JPEG round trip at a quality that is a
        # uniform integer in the closed range JPEG_QUALITY, chroma '420' or '444' (a second launch, sst_jpeg: an all-integer codec,
        # DESIGN.md section 22).  Drawn after the blur and noise parameters, which stay the ones drawn without it.  0: no second launch
        self.DATA.DEGRADE_JPEG_PROB = 0.0
        self.DATA.DEGRADE_JPEG_QUALITY = (30, 95)
        self.DATA.DEGRADE_JPEG_CHROMA = "420"
        # (sigma1, sigma2, theta_deg, noise): validation feeds the generator degrade(gt) with these fixed parameters (key = the image's
        # index, window DEGRADE_BLUR_KSIZE) instead of the LR file; the printed line and _metrics.txt say so.  None: the LR files
        self.DATA.VALIDATE_DEGRADE = None
        # Q in 1..100: validation feeds the generator the JPEG round trip (chroma DEGRADE_JPEG_CHROMA) of its input at this quality -
        # of degrade(gt) with VALIDATE_DEGRADE, else of the plain bicubic LR made from gt; the printed line says so.  None: off
        self.DATA.VALIDATE_DEGRADE_JPEG = None
        # with DEGRADE: the second-order stage of BSRGAN / Real-ESRGAN on the first stage's LR batch (device_data.SecondOrder,
        # sst_filter2d): a second blur at LR resolution with a kernel of a table drawn per epoch - BANK_SIZE
        # kernels, each a sinc (SINC_PROB, cutoff uniform in OMEGA) or of one of the six families of FAMILY_PROB (iso / aniso Gaussian,
        # iso / aniso generalised Gaussian with exponent uniform in BETA_GAUSSIAN, iso / aniso plateau with BETA_PLATEAU), standard
        # deviations uniform in BLUR_SIGMA, on a window that is odd and uniform in 7..KSIZE - applied with BLUR_PROB; noise (NOISE_PROB):
        # Gaussian with a standard deviation uniform in NOISE_SIGMA (0..255 units) or, with SHOT_PROB, signal-dependent with a shot
        # coefficient in SHOT (a heteroscedastic Gaussian, variance s_p * v: Real-ESRGAN's Poisson scale 0.05..2.5, squared, over 256
        # levels; not a Poisson sampler), gray with GRAY_PROB; a JPEG pass (JPEG_PROB, quality a uniform integer in JPEG_QUALITY, chroma
        # DEGRADE_JPEG_CHROMA); and a final sinc filter (FINAL_SINC_PROB, one of SINC_BANK_SIZE kernels with cutoffs uniform in OMEGA)
        # before the JPEG pass with SINC_FIRST_PROB, else after it.  The table is a function of (SEED, epoch); the per-tile draws come
        # from a third private generator, so the first stage's draws are the ones made without it
        self.DATA.DEGRADE_SECOND = False
        self.DATA.DEGRADE2_BLUR_PROB = 0.8
        self.DATA.DEGRADE2_BLUR_SIGMA = (0.2, 1.5)
        self.DATA.DEGRADE2_FAMILY_PROB = (0.45, 0.25, 0.12, 0.03, 0.12, 0.03)
        self.DATA.DEGRADE2_BETA_GAUSSIAN = (0.5, 4.0)
        self.DATA.DEGRADE2_BETA_PLATEAU = (1.0, 2.0)
        self.DATA.DEGRADE2_SINC_PROB = 0.1
        self.DATA.DEGRADE2_NOISE_PROB = 1.0
        self.DATA.DEGRADE2_NOISE_SIGMA = (1.0, 25.0)
        self.DATA.DEGRADE2_SHOT = (1e-5, 0.025)
        self.DATA.DEGRADE2_SHOT_PROB = 0.5
        self.DATA.DEGRADE2_GRAY_PROB = 0.4
        self.DATA.DEGRADE2_FINAL_SINC_PROB = 0.8
        self.DATA.DEGRADE2_OMEGA = (3.141592653589793 / 3, 3.141592653589793)
        self.DATA.DEGRADE2_SINC_FIRST_PROB = 0.5
        self.DATA.DEGRADE2_JPEG_QUALITY = (30, 95)
        self.DATA.DEGRADE2_JPEG_PROB = 1.0
        self.DATA.DEGRADE2_KSIZE = 21
        self.DATA.DEGRADE2_BANK_SIZE = 1024
        self.DATA.DEGRADE2_SINC_BANK_SIZE = 256
        # omega in (0, pi]: validation's input also goes through the sinc filter (kernels.sinc, window DEGRADE2_KSIZE) at this cutoff -
        # after degrade(gt) (or the plain bicubic LR made from gt) and before the VALIDATE_DEGRADE_JPEG stage; the printed line says
        # so.  None: off
        self.DATA.VALIDATE_DEGRADE_SINC = None
        # with DEGRADE_SECOND: the random resize of Real-ESRGAN's second stage (sst_rescale).  Between blur 2 and
        # the final sinc / JPEG a sample is, with the probabilities RESIZE_PROB = (up, down, keep), resized to a scale uniform in
        # [1, RESIZE_RANGE[1]] or [RESIZE_RANGE[0], 1] with a mode uniform in RESIZE_MODES, gets noise 2 at THAT size, and is resized back
        # to the LR size with a mode drawn independently.  The draws come from a fourth private generator: all others stay as they are
        self.DATA.DEGRADE2_RESIZE = False
        self.DATA.DEGRADE2_RESIZE_PROB = (0.3, 0.4, 0.3)
        self.DATA.DEGRADE2_RESIZE_RANGE = (0.3, 1.2)
        self.DATA.DEGRADE2_RESIZE_MODES = ("area", "bilinear", "bicubic")
        # s in [0.25, 2]: validation's input also goes through the resize round trip at this scale, bicubic both ways, no noise - after
        # degrade(gt) (or the plain bicubic LR made from gt) and before the VALIDATE_DEGRADE_SINC stage; the printed line says so.
        # None: off
        self.DATA.VALIDATE_DEGRADE_RESIZE = None
        # with DEGRADE: the random resize of Real-ESRGAN's FIRST stage (sst_blur, sst_rescale_to).  Between the
        # blur and the noise a sample is, with the probabilities RESIZE_PROB = (up, down, keep), resized from the HR size to a scale
        # uniform in [1, RESIZE_RANGE[1]] or [RESIZE_RANGE[0], 1] with a mode uniform in RESIZE_MODES (no antialias), gets its noise at
        # THAT size, and is resized to the LR size with a mode drawn independently - in place of the antialiased bicubic.  Three
        # launches per batch for the one.  The draws come from a fifth private generator: all others stay as they are
        self.DATA.DEGRADE_RESIZE = False
        self.DATA.DEGRADE_RESIZE_PROB = (0.2, 0.7, 0.1)
        self.DATA.DEGRADE_RESIZE_RANGE = (0.15, 1.5)
        self.DATA.DEGRADE_RESIZE_MODES = ("area", "bilinear", "bicubic")
        # (s, m1, m2), s in [0.125, 2]: validation's input is made through the first stage's resize at this scale - blur (with
        # VALIDATE_DEGRADE), resize of gt to the scale s with the mode m1, the noise there, resize to the LR size with m2 - before the
        # other VALIDATE_DEGRADE_* stages in their order; the printed line says so.  None: off
        self.DATA.VALIDATE_DEGRADE_RESIZE1 = None

        self.MODEL = dotdict()
        self.MODEL.G_CONTINUE_FROM_WARMUP = False
        self.MODEL.G_WARMUP_WEIGHTS = ""
        self.MODEL.D_CONTINUE_FROM_WARMUP = False
        self.MODEL.D_WARMUP_WEIGHTS = ""
        self.MODEL.G_IN_CHANNEL = 3
        self.MODEL.G_OUT_CHANNEL = 3
        self.MODEL.G_N_CHANNEL = 64
        self.MODEL.G_N_RCB = 16

        self.MODEL.G_LOSS = dotdict()
        self.MODEL.G_LOSS.VGG19_LAYERS = {"features.17": 1 / 8, "features.26": 1 / 4, "features.35": 1 / 2}
        self.MODEL.G_LOSS.DISC_FEATURES_LOSS_LAYERS = {"features.4": 1 / 4, "features.10": 1 / 2}
        self.MODEL.G_LOSS.CRITERIONS = {"Adversarial": L.BCEWithLogitsLoss()}
        self.MODEL.G_LOSS.CRITERION_WEIGHTS = {
            "Adversarial": 0.001, "ContentVGG": 1.0, "ContentDiscriminator": 2000.0, "Pixel": 1.0,
            "BestBuddy": 50.0, "Gram": 500.0, "PatchwiseST": 100.0, "ST": 1 / 3,
        }
        self.MODEL.G_LOSS.WARMUP_CRITERIONS = {"Pixel": L.MSELoss()}
        self.MODEL.G_LOSS.WARMUP_WEIGHTS = {"Pixel": 1.0}
        self.MODEL.D_IN_CHANNEL = 3
        self.MODEL.D_OUT_CHANNEL = 1
        self.MODEL.D_N_CHANNEL = 64

        self.SOLVER = dotdict()
        self.SOLVER.D_UPDATE_INTERVAL = 100
        self.SOLVER.D_OPTIMIZER = "Adam"
        self.SOLVER.D_BASE_LR = 1e-4
        self.SOLVER.D_BETA1 = 0.9
        self.SOLVER.D_BETA2 = 0.999
        self.SOLVER.D_WEIGHT_DECAY = 0
        self.SOLVER.D_EPS = 1e-4
        self.SOLVER.G_OPTIMIZER = "Adam"
        self.SOLVER.G_BASE_LR = 1e-4
        self.SOLVER.G_BETA1 = 0.9
        self.SOLVER.G_BETA2 = 0.999
        self.SOLVER.G_WEIGHT_DECAY = 0
        self.SOLVER.G_EPS = 1e-4
        # Exponential moving average of the generator's weights, kept by the flat Adam kernel in the same pass (optim.FlatAdam):
        # 0 = off (the step launches what it launches without the option); 0.999 is the usual value.  WARMUP: the decay at Adam
        # step t is min(G_EMA_DECAY, (1 + t) / (10 + t)), so a young average is not dominated by the initial weights.  VALIDATE:
        # the drivers validate, and select "best" on, the averaged generator (engine.g_ema) instead of the last iterate
        self.SOLVER.G_EMA_DECAY = 0.0
        self.SOLVER.G_EMA_WARMUP = True
        self.SOLVER.G_EMA_VALIDATE = True
        # Global gradient-norm clipping and the non-finite step guard, decided on the device inside the flat Adam step
        # (optim.FlatAdam: one fp64 reduction of the flat gradient, then the update on g * min(1, max_norm / (norm + 1e-6))), so they
        # ride in the captured graph without a host sync.  GRAD_CLIP: the maximal global L2 norm per network, 0 = off.
        # SKIP_NONFINITE: an update whose gradient holds a NaN or an infinity is dropped for that network - weights, Adam moments,
        # step counters and the average stay as they were (BatchNorm running statistics do not: the forward pass has moved them
        # already).  All off (default): the step launches what it launches without the options.  Under data parallelism the norm is
        # the averaged gradient's, so every rank decides alike
        self.SOLVER.G_GRAD_CLIP = 0.0
        self.SOLVER.D_GRAD_CLIP = 0.0
        self.SOLVER.SKIP_NONFINITE = False

        self.SCHEDULER = dotdict()
        self.SCHEDULER.STEP_SIZE = self.EXP.N_EPOCHS // 2
        self.SCHEDULER.GAMMA = 0.5
        self.SCHEDULER.MILESTONES = [10]    # reference train.py:80,85 hard-codes MultiStepLR(milestones=[10]) for both optimizers

        # --- additions (not in the reference) ---
        self.DIST = dotdict()
        self.DIST.BACKEND = "nccl"          # RCCL on ROCm; "gloo" in the CPU tests
        self.DIST.BUCKET_D = True           # D grads in two buckets (features / classifier)
        self.DIST.OVERLAP_COMM = True       # hide the gradient all-reduces behind compute (engine.TrainEngine._step_overlapped)
        # RCCL only: the mean-all-reduces are captured INSIDE the iteration's hipGraph (the process group's stream forks from the branch that
        # produced the bucket and is joined into the graph's origin stream) - the iteration stays ONE graph at N > 1.  Off / gloo: the
        # graphs are cut where a collective goes out (_step_overlapped)
        # OFF: built, bit-identical to the cut-graph schedule (tests/test_dp_gpu.py, RCCL world 1), but measured SLOWER on ROCm 7.2: as
        # soon as the graph holds the collectives' nodes the runtime runs its two compute branches one after the other (device stamps:
        # the generator's backward starts when the discriminator branch has ended) - 5.80 ms against 5.20 ms for the cut graphs and
        # 4.97 ms single-process (tools/time_dp.py, three discriminator forwards)
        self.DIST.ONE_GRAPH = os.environ.get("SST_DP_ONE_GRAPH", "0") != "0"
        self.KERNEL = dotdict()
        self.KERNEL.USE_GRAPH = True        # capture the train step into a hipGraph
        self.KERNEL.SYNC_LOSS_EVERY_STEP = False  # reference does .item() per criterion per step (train.py:141)
        # the discriminator step beside the generator's backward, whole iteration = one graph (engine.TrainEngine._iter_gd)
        self.KERNEL.OVERLAP_GD = os.environ.get("SST_OVERLAP_GD", "1") != "0"
        # merged iteration: the conv weight gradients of the discriminator's last backward pass run on the generator's stream after its
        # backward (the discriminator branch is the longer one)
        # (= how many layers, counted from the first: the ones the backward chain reaches last; 0 = none, 8 = all)
        self.KERNEL.DEFER_D_WGRAD = int(os.environ.get("SST_DEFER_D_WGRAD", "8"))
        # merged iteration: D's weight packing on the side stream beside the generator's forward
        self.KERNEL.EARLY_D_PACK = os.environ.get("SST_EARLY_D_PACK", "1") != "0"
        # the discriminator step's D(sr.detach()) forward (train.py:158) is not run again: it repeats the generator step's D(sr)
        # (same input, same weights, deterministic kernels); its running-statistics side effects are replayed (disc_graph.replay_running_stats)
        self.KERNEL.REUSE_D_SR = os.environ.get("SST_REUSE_D_SR", "1") != "0"
        # the discriminator step's two passes, D(gt) and D(sr.detach()) (train.py:155-158), as ONE batch of 2B images with per-pass
        # train-mode BatchNorm statistics (disc_graph.forward on a list of inputs): one launch per layer instead of two, the classifier
        # weight streamed once per direction.  Same values per pass up to fp32 summation order (the weight gradients sum over 2B images in
        # one kernel instead of fl(dW_sr + dW_gt)); applies when the step runs both passes (i.e. not on top of REUSE_D_SR's kept pass)
        self.KERNEL.BATCH_D_STEP = os.environ.get("SST_BATCH_D_STEP", "1") != "0"
        self.KERNEL.LR_ON_DEVICE = False    # True: the LR batch is synthesised from the GT batch on the GPU (sst_bicubic, same
                                            # values as dataset.py:28 on the 1/255 grid) instead of taking the loader's copy

    def add_g_criterion(self, name: str, value, weight: float = 1.0) -> None:
        self.MODEL.G_LOSS.CRITERIONS[name] = value
        self.MODEL.G_LOSS.CRITERION_WEIGHTS[name] = weight

    def remove_g_criterion(self, name: str) -> None:
        if name in self.MODEL.G_LOSS.CRITERIONS:
            del self.MODEL.G_LOSS.CRITERIONS[name]
            del self.MODEL.G_LOSS.CRITERION_WEIGHTS[name]

    def get_all_params(self) -> str:
        params = [getattr(self, attr) for attr in dir(self)
                  if not callable(getattr(self, attr)) and not attr.startswith("__")]
        return str(params)
