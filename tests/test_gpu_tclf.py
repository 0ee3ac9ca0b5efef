"""The target speaker classifier on the GPU: --train_c (Trainer.train(mode='t_classify'), trainer.py:613-642) and the batched
--test_classify (convert.target_classify, convert.py:364-414), against tests/golden/tclf_small.npz (the reference's
TargetClassifier(n_class=3, ns=0.01, dp=0.8, seg_len=128) and one t_classify step; the 10.9 M weights are regenerated from the
seed by oracle.synthetic_patch_sd), the oracle, and the per-fragment Trainer.classify path.

Tolerances.  fp32: those of test_gpu_stage2 for the discriminator (logits 1e-3 of scale, CE 1e-4, every gradient 5e-3 of its
scale on a strided sample of 512 entries and its norm to 5e-3); the clip norm to 5e-3; Adam's first update (about lr * sign(g))
to 0.1 lr on every sampled entry whose gradient is farther from zero than the gradient tolerance (the sign of a sum that
cancels to within rounding is not determined), and never more than lr.  bf16: bounds fitted to the errors measured on an
MI355X (printed by the tests), see TOL."""
import io
import json
import os
import sys
from contextlib import redirect_stdout

import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHANS = (64, 128, 256, 512, 512, 32)

# bf16 (the default dtype of `main.py --train_c`): bf16 storage of every activation through six conv + InstanceNorm2d layers;
# bounds = 2-3 x the errors measured on an MI355X: eval logits 1.2e-2 of scale, CE 6.1e-3 of its value, clip norm 7.0e-4; worst
# weight gradient 0.26 of its tensor's scale (conv6.weight), worst bias gradient 0.45 (conv6.bias: 32 sums over B = 6 samples of
# bf16 rows that largely cancel); no Adam update entry off among those with a determined sign.  The conv biases are not removed by
# InstanceNorm2d (LeakyReLU lies between them, conv_block, model/model.py:211-216): their reference gradients are real (norms 0.17-7.7).
TOL = {'fp32': dict(fwd=1e-3, ce=1e-4, grad_weight=5e-3, gnorm_weight=5e-3, grad_bias=5e-3, gnorm_bias=5e-3, clip=5e-3, upd_off=0.0),
       'bf16': dict(fwd=3e-2, ce=1.5e-2, grad_weight=6e-1, gnorm_weight=6e-1, grad_bias=9e-1, gnorm_bias=9e-1, clip=2e-3,
                    upd_off=0.05)}


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    import zs_amd  # noqa: F401
    return torch.device('cuda:0')


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a - b).max() / max(1e-12, np.abs(b).max())


def _setup(dev, dtype):
    import zs_oracle as O
    from zs_amd.patch import TargetClassifier
    d, m = load_golden('tclf_small.npz')
    T = TargetClassifier(n_class=m['n_class'], ns=m['ns'], dp=m['dp'], seg_len=m['seg_len'], dtype=dtype).to(dev)
    T.load_state_dict(O.synthetic_patch_sd(m['n_class'], m['seed'], seg_len=m['seg_len']))
    return d, m, T


@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
def test_eval_logits_golden(dev, dtype):
    d, m, T = _setup(dev, dtype)
    T.eval()
    lg = T(torch.from_numpy(d['x_eval']).to(dev)).cpu().numpy()              # [B, 513, T], the reference's layout
    e = _rel(lg, d['logits_eval'])
    print('%s eval logits vs reference: %.3g' % (dtype, e))
    assert lg.shape == (3, 3) and e < TOL[dtype]['fwd']


@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
def test_t_classify_step_golden(dev, dtype):
    """One t_classify step (trainer.py:615-628): relabel, train-mode forward with the reference's keep masks, CE, every parameter
    gradient, the clip norm and Adam's first update."""
    from zs_amd.trainer import TclfStep
    d, m, T = _setup(dev, dtype)
    tol = TOL[dtype]
    step = TclfStep(T, m['lr'], m['max_grad_norm'], m['n_speakers'] - m['n_target_speakers'])
    masks = [torch.from_numpy(d['mask.%d' % i]).float().to(dev) for i in range(6)]
    x = torch.from_numpy(d['x_train']).permute(0, 2, 1).contiguous().to(dev)     # [B, T, F]
    c = torch.from_numpy(d['c_raw']).to(dev)
    flat, gflat = T.flat_params()
    before = flat.clone()
    loss, corr = step.step(x, c, masks=masks)
    torch.cuda.synchronize()
    want_corr = int((d['logits_train'].argmax(1) == d['target']).sum())
    clip = float(step.opt.sq.item()) ** 0.5
    print('%s t_classify step: CE %.6f (reference %.6f), clip norm %.5f (%.5f), correct %d (%d)' %
          (dtype, loss.item(), float(d['loss']), clip, float(d['clip_norm']), corr.item(), want_corr))
    assert abs(loss.item() - float(d['loss'])) < tol['ce'] * max(1.0, float(d['loss']))
    assert abs(clip - float(d['clip_norm'])) < tol['clip'] * float(d['clip_norm'])
    if dtype == 'fp32':
        assert corr.item() == want_corr
    worst = {'weight': ('', 0.0), 'bias': ('', 0.0)}
    worst_upd = ('', 0.0)
    upd_all = flat - before
    for k, p in T.named_parameters():
        g = T.grad_view(k).detach().reshape(-1)
        ref, nref = d['g.sample.' + k], float(d['g.norm.' + k])
        got = g[::max(1, g.numel() // 512)][:512].cpu().numpy()
        o = T._zs['offsets'][k]
        u = upd_all[o:o + p.numel()]
        got_u = u[::max(1, u.numel() // 512)][:512].cpu().numpy()
        if k.startswith('conv7.'):                          # unused by the classifier: no gradient, no update
            assert nref == 0.0 and float(g.abs().max()) == 0.0 and float(u.abs().max()) == 0.0
            continue
        kind = 'bias' if k.endswith('.bias') else 'weight'
        e = np.abs(got - ref).max() / max(1e-9, np.abs(ref).max())
        en = abs(g.double().norm().item() - nref) / max(1e-9, nref)
        if max(e, en) > worst[kind][1]:
            worst[kind] = (k, max(e, en))
        assert e < tol['grad_' + kind] and en < tol['gnorm_' + kind], (k, e, en)
        # Adam's first step is about lr * sign(g): an entry whose gradient lies within the gradient tolerance of zero (a sum that
        # cancels) may take either sign; every other entry must match to 0.1 lr
        sure = np.abs(ref) > tol['grad_' + kind] * np.abs(ref).max()
        off = float((np.abs(got_u - d['upd.sample.' + k])[sure] > 0.1 * m['lr']).mean()) if sure.any() else 0.0
        if off > worst_upd[1]:
            worst_upd = (k, off)
        assert off <= tol['upd_off'], (k, off)
        assert float(u.abs().max()) <= 1.01 * m['lr']
    print('%s worst gradient error (relative to the tensor\'s scale, sample / norm): weights %s %.3g, biases %s %.3g; worst share of '
          'Adam-update entries off by > 0.1 lr: %s %.3g' % ((dtype,) + worst['weight'] + worst['bias'] + worst_upd))


def _small_hps(tmp_path, **kw):
    from zs_amd.hps import make_hps
    hps = make_hps(enc_size=8, emb_size=32, n_speakers=102, n_target_speakers=2, batch_size=4, tclf_iters=3, **kw)
    p = str(tmp_path / 'hps.json')
    json.dump(hps._asdict(), open(p, 'w'))
    return hps, p


def test_train_t_classify_checkpoint(dev, tmp_path, monkeypatch):
    from zs_amd.dataloader import DataLoader, SyntheticDataset
    from zs_amd.trainer import Trainer
    monkeypatch.setenv('ZS_CKPT_EVERY', '3')
    monkeypatch.setenv('ZS_LOG_EVERY', '1')
    hps, _ = _small_hps(tmp_path)
    loader = DataLoader(SyntheticDataset(64, seg_len=128, n_speakers=102), hps.batch_size)
    tr = Trainer(hps, loader, 'targeted_residual', 'multilabel_binary', log_dir=str(tmp_path / 'log'), dtype='bf16', device=dev)
    w0 = tr.TargetClassifier.flat_params()[0].clone()
    buf = io.StringIO()
    with redirect_stdout(buf):
        tr.train(str(tmp_path / 'model.pth'), 'train', mode='t_classify')
    assert 'Target Classifier:[00003/00003], acc=' in buf.getvalue()
    assert not torch.equal(w0, tr.TargetClassifier.flat_params()[0])                 # the classifier was stepped
    ck = torch.load(str(tmp_path / 'model.pth-tclf-3'), map_location='cpu', weights_only=True)
    sd = ck['target_classifier']
    assert sd and all(k.startswith('module.') for k in sd) and 'module.conv_classify.weight' in sd
    tr2 = Trainer(hps, None, 'targeted_residual', 'multilabel_binary', log_dir=str(tmp_path / 'log'), dtype='bf16', device=dev)
    with redirect_stdout(io.StringIO()):
        tr2.load_model(str(tmp_path / 'model.pth-tclf-3'), 'encoder, decoder, generator, target_classifier')
    assert tr2.tclf_loaded
    assert torch.equal(tr2.TargetClassifier.flat_params()[0], tr.TargetClassifier.flat_params()[0])


def test_train_t_classify_rejects_bad_labels_and_naive(dev, tmp_path):
    from zs_amd.dataloader import DataLoader, SyntheticDataset
    from zs_amd.hps import make_hps
    from zs_amd.trainer import Trainer
    hps = make_hps(enc_size=8, emb_size=32, n_speakers=4, n_target_speakers=2, batch_size=4, tclf_iters=1)
    loader = DataLoader(SyntheticDataset(16, seg_len=128, n_speakers=4), 4)
    tr = Trainer(hps, loader, 'targeted_residual', 'multilabel_binary', log_dir=str(tmp_path / 'log'), dtype='fp32', device=dev)
    w0 = tr.TargetClassifier.flat_params()[0].clone()
    with pytest.raises(ValueError):
        tr.train(str(tmp_path / 'model.pth'), 'train', mode='t_classify')
    assert tr.tclf is None and torch.equal(w0, tr.TargetClassifier.flat_params()[0])       # raised before the first step
    hps2 = make_hps(enc_size=8, emb_size=32, n_speakers=102, n_target_speakers=2, batch_size=4, tclf_iters=1)
    tr2 = Trainer(hps2, loader, 'naive', 'multilabel_binary', log_dir=str(tmp_path / 'log'), dtype='fp32', device=dev)
    with pytest.raises(ValueError, match='naive'):
        tr2.train(str(tmp_path / 'model.pth'), 'train', mode='t_classify')


def test_main_train_c_synthetic(dev, tmp_path, monkeypatch, capsys):
    """`python main.py --train_c --synthetic` (main.py:165-167): the stage-1 loader over all speakers, mode t_classify."""
    sys.path.insert(0, ROOT)
    import main
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv('ZS_CKPT_EVERY', '2')
    from zs_amd.hps import make_hps
    hps = make_hps(enc_size=8, emb_size=32, n_speakers=102, n_target_speakers=2, batch_size=2, tclf_iters=2)
    p = str(tmp_path / 'hps.json')
    json.dump(hps._asdict(), open(p, 'w'))
    main.main(['--train_c', '--synthetic', '--hps_path', p, '--ckpt_dir', str(tmp_path / 'ck'), '--dtype', 'bf16'])
    out = capsys.readouterr().out
    assert 'Target Classifier:[00002/00002], acc=' in out and 'pre_AE' not in out and 'patch_G' not in out
    assert os.path.exists(str(tmp_path / 'ck' / 'model.pth-tclf-2'))


def _classify_trainer(dev, tmp_path, dtype='fp32'):
    import zs_oracle as O
    from zs_amd.hps import make_hps
    from zs_amd.trainer import Trainer
    torch.manual_seed(3)
    hps = make_hps(enc_size=16, emb_size=32, n_speakers=4, n_target_speakers=2)
    tr = Trainer(hps, None, 'targeted_residual', 'multilabel_binary', log_dir=str(tmp_path / 'log'), dtype=dtype, device=dev)
    sd = O.synthetic_patch_sd(3, seed=29)
    tr.TargetClassifier.load_state_dict(sd)
    return tr, sd


def test_classify_batch_equals_per_fragment_classify_and_oracle(dev, tmp_path):
    import zs_oracle as O
    from zs_amd import convert as cv
    tr, sd = _classify_trainer(dev, tmp_path)
    rng = np.random.RandomState(5)
    lengths = [129, 700, 255, 256, 257, 383, 384, 385, 511, 640, 300, 150]
    specs = [np.clip(rng.rand(n, 513).astype(np.float32), 1e-8, 1.0) for n in lengths]
    logits, plan = cv.classify_batch(specs, tr, 128, max_batch=5)            # chunks of 5 and a remainder
    lg = logits.cpu().numpy()
    assert plan == cv.tclf_plan(lengths, 128) and lg.shape == (len(plan), 3) and len(plan) > 20
    # the same from a padded device batch (the target_classify path)
    T_max = max(lengths)
    mag = torch.zeros(len(specs), T_max, 513, device=dev)
    for i, s in enumerate(specs):
        mag[i, :len(s)] = torch.from_numpy(s)
    lg2, plan2 = cv.classify_batch((mag, lengths), tr, 128)
    assert plan2 == plan
    ref = np.concatenate([tr.classify(specs[u][s:s + 128][None]) for u, s in plan], axis=0)
    e1, e2 = _rel(lg, ref), _rel(lg2.cpu().numpy(), ref)
    print('classify_batch vs per-fragment Trainer.classify: %.3g (list), %.3g (device batch)' % (e1, e2))
    assert e1 < 1e-5 and e2 < 1e-5
    assert (lg.argmax(1) == ref.argmax(1)).all() and (lg2.cpu().numpy().argmax(1) == ref.argmax(1)).all()
    sd_clf = {k: v for k, v in sd.items() if not k.startswith('conv7.')}
    pick = list(range(0, len(plan), max(1, len(plan) // 6)))
    xs = torch.from_numpy(np.stack([specs[plan[i][0]][plan[i][1]:plan[i][1] + 128] for i in pick])).permute(0, 2, 1)
    with torch.no_grad():
        _, o = O.patch_discriminator_forward(sd_clf, xs, 0.01, 128, classify=True, training=False)
    e3 = _rel(lg[pick], o.numpy())
    print('classify_batch vs oracle (fp32): %.3g' % e3)
    assert e3 < 1e-3


def test_frag_gather_bit_exact(dev):
    from zs_amd import _lib as L
    g = torch.Generator(device=dev).manual_seed(4)
    n_utt, T_max, seg = 3, 301, 128
    stride = T_max * 513 + 3                                                 # utterances not 16-byte aligned either
    src = torch.rand(n_utt * stride + 8, generator=g, device=dev)
    table = [(0, 0), (0, 1), (1, 7), (2, 173), (1, 3), (2, 2), (0, 173), (1, 99), (5, 0), (0, 200)]   # last two: invalid -> zeros
    n_frag = len(table)
    dst_buf = torch.full((n_frag * seg * 513 + 4,), -7.0, device=dev)
    tab = torch.tensor(table, dtype=torch.int32, device=dev)
    for off in (0, 1, 2, 3):                                                   # destination phase inside a 16-byte word
        dst = dst_buf[off:off + n_frag * seg * 513]
        st = torch.cuda.current_stream(dev).cuda_stream
        L.call('zs_frag_gather', 'ZsFragGather', st, src=L.ptr(src), utt_stride=stride, n_utt=n_utt, T_max=T_max, table=L.ptr(tab),
               n_frag=n_frag, seg_len=seg, dst=L.ptr(dst))
        got = dst.view(n_frag, seg, 513)
        for f, (u, s) in enumerate(table):
            if u < n_utt and s + seg <= T_max:
                want = src[u * stride:u * stride + T_max * 513].view(T_max, 513)[s:s + seg]
                assert torch.equal(got[f], want), (off, f)
            else:
                assert not got[f].any(), (off, f)
        assert float(dst_buf[off + n_frag * seg * 513]) == -7.0                # nothing written past the batch
        dst_buf.fill_(-7.0)


def test_tclf_score_counts(dev):
    from zs_amd import _lib as L
    rng = np.random.RandomState(8)
    n = 1000
    lg = rng.randint(-2, 3, size=(n, 3)).astype(np.float32)                  # many ties
    host = np.zeros((n, 32), np.float32)
    host[:, :3] = lg
    host[:, 3:] = 99.0                                                         # columns past the third are never read
    tgt = rng.randint(-1, 3, size=n).astype(np.int32)
    pred_want = lg.argmax(1)
    d_lg, d_t = torch.from_numpy(host).to(dev), torch.from_numpy(tgt).to(dev)
    pred = torch.full((n,), -5, dtype=torch.int32, device=dev)
    cnt = torch.tensor([10, 20], dtype=torch.int32, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    for _ in range(2):
        L.call('zs_tclf_score', 'ZsTclfScore', st, logits=L.ptr(d_lg), ld=32, target=L.ptr(d_t), n_frag=n, pred=L.ptr(pred),
               correct=L.ptr(cnt), count=L.ptr(cnt, 1))
    assert np.array_equal(pred.cpu().numpy(), pred_want)
    correct = int((pred_want == tgt).sum())
    assert cnt.cpu().tolist() == [10 + 2 * correct, 20 + 2 * n]


def _wav(rng, n):
    t = np.arange(n) / 16000.0
    y = 0.3 * np.sin(2 * np.pi * rng.uniform(100, 3000) * t) + 0.1 * np.sin(2 * np.pi * rng.uniform(3000, 7000) * t) + 0.05 * rng.randn(n)
    return (np.clip(y, -1, 1) * 32767).astype(np.int16)


def test_main_test_classify_end_to_end(dev, tmp_path, monkeypatch, capsys):
    """`python main.py --test_classify --ckpt_pth A --load_tclf_model_name B` (main.py:196-199): the accuracy equals a host loop over
    Trainer.classify per fragment with the classifier of checkpoint B."""
    from scipy.io import wavfile
    sys.path.insert(0, ROOT)
    import main
    from zs_amd import convert as cv
    from zs_amd.hps import make_hps
    from zs_amd.preprocess import get_spectrograms, load_wav
    rng = np.random.RandomState(17)
    res = tmp_path / 'result'
    wdir = res / 'english' / 'test'
    wdir.mkdir(parents=True)
    lines = []
    for i, (src, tar, n) in enumerate([('S015', 'V001', 60000), ('S015', 'V002', 90000), ('S130', 'V001', 140000),
                                       ('S130', 'V002', 27000), ('S089', 'V001', 45000), ('S089', 'V002', 110000)]):
        utt = '%04d' % (i + 1)
        wavfile.write(str(wdir / ('%s_%s.wav' % (tar, utt))), 16000, _wav(rng, n))
        lines.append('test/%s_%s %s' % (src, utt, tar))
    syn = str(tmp_path / 'synthesis.txt')
    open(syn, 'w').write('\n'.join(lines) + '\n')
    hps = make_hps(enc_size=16, emb_size=32, n_speakers=4, n_target_speakers=2,
                   load_model_list='encoder, decoder, generator, target_classifier')
    hps_path = str(tmp_path / 'hps.json')
    json.dump(hps._asdict(), open(hps_path, 'w'))
    tr_a, _ = _classify_trainer(dev, tmp_path)
    tr_a.save_model(str(tmp_path / 'A.pth'), 's2', 1)                        # checkpoint A: classifier of seed 29
    w_a = tr_a.TargetClassifier.flat_params()[0].clone()
    import zs_oracle as O
    tr_a.TargetClassifier.load_state_dict(O.synthetic_patch_sd(3, seed=31))
    tr_a.save_model(str(tmp_path / 'B.pth'), 'tclf', 1)                      # checkpoint B: classifier of seed 31
    A, B = str(tmp_path / 'A.pth-s2-1'), str(tmp_path / 'B.pth-tclf-1')
    seen = {}
    real = cv.classify_batch

    def spy(specs, trainer, seg_len, max_batch=256):
        seen['w'] = trainer.TargetClassifier.flat_params()[0].clone()
        return real(specs, trainer, seg_len, max_batch=max_batch)
    monkeypatch.setattr(cv, 'classify_batch', spy)
    capsys.readouterr()
    main.main(['--test_classify', '--ckpt_pth', A, '--load_tclf_model_name', B, '--hps_path', hps_path, '--synthesis_list', syn,
               '--result_dir', str(res), '--sub_result_dir', 'english', '--dtype', 'fp32'])
    out = capsys.readouterr().out
    got = [l for l in out.split('\n') if l.startswith('Classification Acc: ')]
    assert len(got) == 1 and 'warning' not in out
    # the host loop of the reference (convert.py:370-413) with a trainer that took its classifier from B
    from zs_amd.convert import get_trainer
    with redirect_stdout(io.StringIO()):
        tr_b = get_trainer(hps_path, A, 'targeted_residual', 'multilabel_binary', B)
    assert torch.equal(seen['w'], tr_b.TargetClassifier.flat_params()[0])             # the weights of checkpoint B were used,
    assert not torch.equal(seen['w'], w_a)                                             # not those of A
    acc = []
    for line in lines:
        utt, tar = line.split(' ')[0].split('/')[1].split('_')[1], line.split(' ')[1]
        _, spec = get_spectrograms(str(wdir / ('%s_%s.wav' % (tar, utt))))
        for u, s in cv.tclf_plan([len(spec)], 128):
            logit = tr_b.classify(spec[s:s + 128][None])[0]
            acc.append(int(cv.tclf_predict(logit[None])[0] == tar))
    want = 'Classification Acc: {:.3f}'.format(np.sum(acc) / float(len(acc)))
    print('test_classify: %s (host loop: %s over %d fragments)' % (got[0], want, len(acc)))
    assert got[0] == want
    # without target_classifier in load_model_list: one warning line, the classifier is not loaded
    hps2 = make_hps(enc_size=16, emb_size=32, n_speakers=4, n_target_speakers=2)
    hps2_path = str(tmp_path / 'hps2.json')
    json.dump(hps2._asdict(), open(hps2_path, 'w'))
    main.main(['--test_classify', '--ckpt_pth', A, '--load_tclf_model_name', B, '--hps_path', hps2_path, '--synthesis_list', syn,
               '--result_dir', str(res), '--sub_result_dir', 'english', '--dtype', 'fp32'])
    out2 = capsys.readouterr().out
    assert sum('warning' in l for l in out2.split('\n')) == 1 and 'Classification Acc: ' in out2
    assert not torch.equal(seen['w'], tr_b.TargetClassifier.flat_params()[0])


def test_target_classify_synchronises_once(dev, tmp_path):
    """target_classify enqueues the spectrograms, the gather, the forwards and the scoring without waiting for the device: the
    read of the two counts at the end is its only synchronising torch operation (torch's sync debug mode flags every one:
    blocking copies from pageable memory, .item(), .cpu())."""
    import warnings
    from scipy.io import wavfile
    from zs_amd import convert as cv
    rng = np.random.RandomState(23)
    wdir = tmp_path / 'result' / 'test'
    wdir.mkdir(parents=True)
    lines = []
    for i, (tar, n) in enumerate([('V001', 50000), ('V002', 80000), ('V001', 120000), ('S015', 33000)]):
        utt = '%04d' % (i + 1)
        wavfile.write(str(wdir / ('%s_%s.wav' % (tar, utt))), 16000, _wav(rng, n))
        lines.append('test/S130_%s %s' % (utt, tar))
    syn = str(tmp_path / 'synthesis.txt')
    open(syn, 'w').write('\n'.join(lines) + '\n')
    tr, _ = _classify_trainer(dev, tmp_path)
    with redirect_stdout(io.StringIO()):
        acc0 = cv.target_classify(tr, 128, syn, str(tmp_path / 'result'))          # first use: engine and buffers
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('warn')
    try:
        with warnings.catch_warnings(record=True) as w, redirect_stdout(io.StringIO()):
            warnings.simplefilter('always')
            acc = cv.target_classify(tr, 128, syn, str(tmp_path / 'result'))
    finally:
        torch.cuda.set_sync_debug_mode('default')
    syncs = [str(x.message) for x in w if 'synchroniz' in str(x.message)]
    print('synchronising operations in target_classify: %d' % len(syncs))
    assert acc == acc0 and len(syncs) == 1, syncs
