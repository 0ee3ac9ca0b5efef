"""The plan of the fused optimizer step (zs_amd.optim.plan_jobs / check_cover) on the host: the job list must cover a net's flat
parameter buffer exactly once.  Parameter shapes only: no GPU is touched."""
import pytest
import torch


def _nets():
    import zs_amd  # noqa: F401
    from zs_amd.model import Decoder, Encoder
    E, ch, nspk = 1024, 1024, 102                  # the benchmark's Encoder / Decoder
    return (Encoder(ns=0.01, dp=0.5, enc_size=E, seg_len=128, enc_mode='multilabel_binary', dtype='bf16'),
            Decoder(ns=0.01, c_in=E, c_h=ch, c_a=nspk, seg_len=128, dtype='bf16'))


def test_check_cover_raises_on_an_overlap_and_on_a_hole():
    from zs_amd import _lib as L
    from zs_amd.optim import check_cover
    good = [dict(kind='weight', off=0, len=40), dict(kind='range', off=40, len=8), dict(kind='vector', off=48, len=16)]
    check_cover(good, 64)
    with pytest.raises(L.ZsError, match='overlap'):
        check_cover([good[0], dict(kind='range', off=36, len=12), good[2]], 64)
    with pytest.raises(L.ZsError, match='hole'):
        check_cover([good[0], dict(kind='range', off=44, len=4), good[2]], 64)
    with pytest.raises(L.ZsError, match='hole'):
        check_cover(good[1:], 64)
    with pytest.raises(L.ZsError, match='of a buffer of 68'):
        check_cover(good, 68)
    with pytest.raises(L.ZsError):
        check_cover([good[1], good[0], good[2]], 64)          # not sorted


@pytest.mark.parametrize('dtype', ['bf16', 'fp32'])
def test_bench_size_plans_cover_the_flat_buffers(dtype):
    """Encoder and Decoder at the benchmark's size: every GEMM-operand weight is a weight job, the re-ordered biases are vector
    jobs, nothing is left to a re-pack behind the launch, and the list passes the cover check."""
    from zs_amd.optim import check_cover
    for net in _nets():
        jobs, rest_w, rest_v = net.adam_pack_jobs(dtype)
        n = net.flat_params()[0].numel()
        check_cover(jobs, n)
        assert not rest_w and not rest_v
        offs = net._zs['offsets']
        by_off = {j['off']: j for j in jobs}
        for name, p in net.named_parameters():
            if name.endswith('.weight') and not name.startswith('emb') or 'weight_' in name:
                j = by_off[offs[name]]
                assert j['kind'] == 'weight' and j['len'] == p.numel(), name
            elif 'RNN.bias' in name:
                assert by_off[offs[name]]['kind'] == 'vector', name
        assert sum(j['len'] for j in jobs) == n and len(jobs) <= 256
        # an overlap or a hole made in this list is caught too
        k = next(i for i, j in enumerate(jobs) if j['kind'] == 'range')
        with pytest.raises(Exception, match='overlap|hole'):
            check_cover(jobs[:k] + [dict(jobs[k], len=jobs[k]['len'] - 4)] + jobs[k + 1:], n)
        with pytest.raises(Exception, match='overlap|hole'):
            check_cover(jobs[:k] + [dict(jobs[k], len=jobs[k]['len'] + 4)] + jobs[k + 1:], n)


def test_plan_sends_what_it_cannot_express_to_the_rest():
    """A weight with more taps than the fused kernel's tiles take, and `raw` views, go to the re-pack behind the launch; the
    parameter itself is then updated by a range job."""
    from zs_amd.layers import weight_operand, weight_view
    from zs_amd.optim import plan_jobs
    flat = torch.zeros(8 * 4 * 9 + 8 + 16 * 4)
    w9 = flat[:288].view(8, 4, 9)
    w1 = flat[296:360].view(16, 4)
    buf = torch.zeros(1, device='meta')
    view = weight_view(buf, 0, 64, 64, 128, 64)
    ops = [weight_operand(w9, 8, 4, 9, (36, 9, 1), [view]),
           weight_operand(w1, 16, 4, 1, (4, 1, 0), [view], raw=[dict(taps=1)])]
    jobs, rest_w, rest_v = plan_jobs(flat, ops, [])
    assert [(j['kind'], j['off'], j['len']) for j in jobs] == [('range', 0, 296), ('weight', 296, 64)]
    assert len(rest_w) == 2 and rest_w[0] is ops[0] and rest_w[1]['views'] == [] and rest_w[1]['raw'] == [dict(taps=1)]
