"""TrainEngine's captured iteration against the eager one, shared by tests/test_patch_loss_fp64_gpu.py and
tests/test_content_losses_fp64_gpu.py: Adversarial + Pixel + ST + the given criteria at their reference weights
(MODEL.G_LOSS.CRITERION_WEIGHTS) on a small model (G 16 channels / 2 blocks, D 8 channels, B = 4, 96 px), 5 iterations, D updated
every iteration.  Generator and discriminator state dicts and the reported loss values must come out equal bit for bit."""
import torch


def graph_vs_eager(criteria, reuse_d_sr, after_first_eager_step=None):
    """criteria(cfg) -> [(name, module)], built after G and D from the same RNG stream in both runs.
    reuse_d_sr: the discriminator step reuses the generator step's D(sr) pass (KERNEL.REUSE_D_SR); otherwise D(gt) and D(sr.detach())
    run as one batch (KERNEL.BATCH_D_STEP).  after_first_eager_step(eng, cfg, gt): called in the eager run after its first step."""
    from srganst.config import Config
    from srganst.engine import TrainEngine
    from srganst.loss import MSELoss, StructureTensorLoss
    from srganst.model import Discriminator, Generator

    def run(use_graph):
        cfg = Config()
        cfg.MODEL.G_N_CHANNEL, cfg.MODEL.G_N_RCB, cfg.MODEL.D_N_CHANNEL = 16, 2, 8
        cfg.KERNEL.REUSE_D_SR, cfg.KERNEL.BATCH_D_STEP = reuse_d_sr, True
        torch.manual_seed(1)
        D, G = Discriminator(cfg).cuda().train(), Generator(cfg).cuda().train()
        cfg.add_g_criterion("Pixel", MSELoss(), 1.0)
        cfg.add_g_criterion("ST", StructureTensorLoss(), 1 / 3)
        names = []
        for name, crit in criteria(cfg):
            cfg.add_g_criterion(name, crit, cfg.MODEL.G_LOSS.CRITERION_WEIGHTS[name])
            names.append(name)
        cfg.SOLVER.D_UPDATE_INTERVAL = 1
        eng = TrainEngine(cfg, G, D, use_graph=use_graph, adam_capturable=True)
        gen = torch.Generator().manual_seed(2)
        for it in range(5):
            gt = torch.rand(4, 3, 96, 96, generator=gen).cuda()
            lr = torch.rand(4, 3, 24, 24, generator=gen).cuda()
            eng.step(gt, lr)
            if it == 0 and not use_graph and after_first_eager_step is not None:
                after_first_eager_step(eng, cfg, gt)
        torch.cuda.synchronize()
        assert eng.graph_active == use_graph
        for name in names:
            assert name in eng.loss_values
        return G.state_dict(), D.state_dict(), {k: v.item() for k, v in eng.loss_values.items()}

    g1, d1, l1 = run(False)
    g2, d2, l2 = run(True)
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k
    for k in d1:
        assert torch.equal(d1[k], d2[k]), k
    assert l1 == l2, (l1, l2)
