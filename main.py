"""Command line of the autoencoder hot path, with the reference's flag names (main.py:27-79):

  python main.py --preprocess [--remake]                  (wav directories -> dataset container + index JSONs)
  python main.py --train_ae [--load_model] [--hps_path hps/zerospeech_english_1024.json] [--synthetic]
  python main.py --train_p | --train_tgat [--load_model] [--synthetic]     (stage 2: patchGAN from an ae checkpoint)
  python main.py --test --enc_only | --test_encode        (needs the preprocessed HDF5 + a checkpoint)
  python main.py --test_single --s_speaker S015 --t_speaker V002 [--enc_only]      (one wav -> result.wav + result.txt)
  python main.py --cross_test [--enc_only]                 (every test utterance to every V* speaker, batched)
  python main.py --train_c [--load_model] [--synthetic]    (the target speaker classifier, mode t_classify)
  python main.py --test_classify --load_tclf_model_name CKPT   (scores the wavs --test wrote; hps load_model_list must name
                                                           target_classifier)
  python main.py --convert_dir DIR --t_speaker V001,V002 [--enc_only] [--ckpt_pth CKPT]    (every *.wav of DIR, any format and
                                                           rate, to each target: {result_dir}/{sub_result_dir}/convert/
                                                           {target}/{stem}.wav + .txt and convert_dir.json)
  python main.py --synth_dir DIR --t_speaker V001,V002 [--enc_only] [--ckpt_pth CKPT]      (every *.txt of DIR, unit files as
                                                           --test_encode / --convert_dir write them, spoken by each target:
                                                           {result_dir}/{sub_result_dir}/synth/{target}/{stem}.wav and
                                                           synth_dir.json)

Vocoder of --test, --cross_test, --test_single, --convert_dir and --synth_dir: --gl_iters N sets the Griffin-Lim iterations (hp.n_iter,
default 300), --gl_momentum A in [0, 1) the fast Griffin-Lim momentum (hp.gl_momentum, default 0: the reference's plain loop), e.g.
`--gl_iters 100 --gl_momentum 0.99`.  --out_sr N writes their wavs at N Hz instead of 16000 (hp.out_sr; band-limited resampling
on the GPU, zs_amd.resample), e.g. `--out_sr 44100`; N / 16000 must lie within [1/32, 32].

Sound files read by --preprocess, --test_single, --test_classify and --convert_dir may have any sample rate: they are resampled
to 16 kHz on the GPU as the reference's librosa.load does.

Every --train* mode takes --device_data: the training set is uploaded into GPU memory once and each batch is gathered there
(zs_amd.pool), in the host DataLoader's order; ZS_POOL_MAX_GB caps the pool's size.

--resume with exactly one of --train_ae, --train_p, --train_tgat, --train_c (with or without --device_data): every checkpoint gets
a train-state file (<ckpt_dir>/train_state/, zs_amd.resume) and the run continues bit for bit from the newest one in --ckpt_dir,
or from iteration 0 when there is none: the same command starts a run and restarts it after an interruption.

--ema D with any --train* mode (D in [0, 1), e.g. 0.999): every optimizer keeps an exponential moving average of its net's weights,
updated inside the Adam kernels; every checkpoint then carries `<net>_ema` entries beside the raw weights, and --resume continues the
averages bit for bit.  --use_ema with --test, --cross_test, --test_encode, --test_single, --test_classify, --convert_dir or --synth_dir
converts with the averaged weights of the checkpoint; with --load_model a training run starts from them, e.g. stage 2 from the
averaged autoencoder: `--train_tgat --load_model --use_ema --ema 0.999`.  Where a flag would have no effect (--ema without a
training mode, --use_ema without a mode that loads a checkpoint) it is refused before anything is built.

--valid_every N with --train_ae or --train (zs_amd.validation): after every N-th iteration of the pretrain_AE stage, and after its
last one, the autoencoder is run forward on a held-out set that lies in GPU memory -- --valid_batches M batches (default 8) of
hps.batch_size segments, always the same data with the same noise -- and the reconstruction loss (overall, over the target speakers,
the worst speaker), the entropy, dead count and flip rate of the unit bits are logged, printed and appended, with the per-speaker
table, to <ckpt_dir>/valid.jsonl; the checkpoint with the lowest loss so far is kept as <model_name>-ae-best, outside the
max_to_keep window.  The set: --valid_index_path PATH (an index JSON as --preprocess writes, over --dataset_path, group --valid_flag,
default train), or --valid_holdout K (every K-th utterance of --index_path leaves the training set and becomes the validation
set), or, with --synthetic and neither, a synthetic set of its own.  The training run computes bit for bit what it computes without
validation, and --resume continues the records and the best value; a run without --resume starts from iteration 0 and so
empties an existing valid.jsonl in --ckpt_dir and overwrites -ae-best, as it overwrites the numbered checkpoints:
  python main.py --train_ae --synthetic --valid_every 1000
  python main.py --train_ae --valid_every 1000 --valid_holdout 20 --resume --ema 0.999

--adapt_voice NAME --adapt_dir DIR --ckpt_pth CKPT (zs_amd.voice): enrol a voice that was not in the training run.  The *.wav of DIR
(read as --convert_dir reads them) are encoded once by the frozen Encoder, and the five embedding rows through which the Decoder sees
a speaker are fitted to them -- random seg_len-frame segments, the L1 reconstruction loss, Adam(lr hps.lr or --adapt_lr, betas
(0.5, 0.9)) and the run's gradient clip over the five rows, every other weight frozen -- for --adapt_iters iterations (default 500),
starting from the rows of speaker --adapt_init or, without it, from the mean of each table.  The result is {voice_dir}/NAME.voice.npz
(--voice_dir, default {ckpt_dir}/voices); no checkpoint, hps or speaker2id file is written, and the same command on the same files
gives the same rows bit for bit.  --voice NAME=FILE (repeatable) with --convert_dir or --synth_dir and --enc_only appends such voices
to the Decoder's tables, and --t_speaker may then name them (speaker2id is looked up first).  Voices convert through the autoencoder
alone: the stage-2 Generator has rows for its trained target speakers only, so --voice without --enc_only is refused, as is every
other combination without effect, before anything is built:
  python main.py --adapt_voice ANNA --adapt_dir wavs/ --ckpt_pth CKPT --adapt_init V001
  python main.py --convert_dir in/ --enc_only --voice ANNA=ckpt_english/voices/ANNA.voice.npz --t_speaker ANNA,V001 --ckpt_pth CKPT

--fit_codebook K --fit_dir DIR [--codebook_out FILE] [--codebook_iters N] [--codebook_seed S] (zs_amd.codebook), with --ckpt_pth or
the usual model flags and --use_ema: the *.wav of DIR (read as --convert_dir reads them) are encoded, the *.txt unit files of DIR are
added, and K codewords are fitted to all their units by k-modes on the GPU; the codebook goes to FILE (default
{ckpt_dir}/codebooks/K<K>.codebook.npz) with a fit_codebook.json beside it.  --codebook FILE with --convert_dir, --synth_dir or
--test_encode snaps every unit to its nearest codeword before it is written and before the Decoder sees it: unit files become
sequences over at most K symbols, each gets a sibling <name>.idx.txt with one codeword index per line, and convert_dir.json /
synth_dir.json gain a 'codebook' entry (--synth_dir also writes the snapped units beside each wav):
  python main.py --fit_codebook 1024 --fit_dir wavs/ --ckpt_pth CKPT
  python main.py --convert_dir in/ --t_speaker V001 --ckpt_pth CKPT --codebook ckpt_english/codebooks/K1024.codebook.npz
With --enc_mode continues the same flags take the vector path (zs_amd.vq): --fit_codebook fits K real-valued codewords to the
encoder's rows of the *.wav of DIR by k-means (default {ckpt_dir}/codebooks/K<K>.vq.npz; *.txt are ignored), --codebook FILE.vq.npz
snaps every encoded frame to its nearest codeword in Euclidean distance before the Decoder sees it and writes <name>.idx.txt, and
--synth_dir --codebook FILE.vq.npz speaks the *.idx.txt files of a folder (one integer per line).  The file's kind and the model's
enc_mode must agree:
  python main.py --enc_mode continues --fit_codebook 1024 --fit_dir wavs/ --ckpt_pth CKPT
  python main.py --enc_mode continues --convert_dir in/ --t_speaker V001 --ckpt_pth CKPT --codebook ckpt_english/codebooks/K1024.vq.npz
  python main.py --enc_mode continues --synth_dir idx/ --t_speaker V001 --ckpt_pth CKPT --codebook ckpt_english/codebooks/K1024.vq.npz

--vq_train FILE.vq.npz with --train_ae and --enc_mode continues (zs_amd.vq_train): the autoencoder is trained through that vector
codebook -- every encoder row of a batch is snapped to its nearest codeword in front of the Decoder, whose input gradient passes
straight through; --vq_beta B (default 0.25, in (0, 10]) weighs the commitment term that keeps the encoder near its codewords, and the
codebook follows the encoder by an exponential moving average of decay --vq_decay D (default 0.99, in [0, 1)).  The log gains loss_vq,
the share of codewords used and the perplexity; every checkpoint gets <checkpoint>.vq.npz beside it, the file --codebook reads.
--vq_restart T (in (0, 1); off by default) puts a codeword that took no row of the batch and whose averaged count fell below T back
onto one of the batch's encoder rows, on the device inside the step; the log then ends with the restarts so far.
--ema, --device_data and --load_model combine with it; --resume, --valid_every, a multi-rank launch and every other --train* mode are
refused before anything is built:
  python main.py --enc_mode continues --train_ae --load_model --vq_train ckpt_english/codebooks/K1024.vq.npz

--fit_codebook K --rvq S with --enc_mode continues (zs_amd.rvq): a residual codebook of S stages (2 to 8) of K codewords each, stage s
fitted to what stage s - 1 left over; the file (default {ckpt_dir}/codebooks/K<K>x<S>.rvq.npz) gives a frame S indices, S log2 K bits,
and its first s of them are a valid coarser description.  --codebook FILE.rvq.npz takes it wherever a vector codebook goes, and
--rvq_stages s uses its first s stages: --convert_dir and --test_encode write <name>.idx.txt with s indices per line (default: all
S), --synth_dir speaks the first s columns of every *.idx.txt (default: the columns a file has) and refuses a file with fewer.
--vq_train refuses a residual codebook, as every flag here is refused without its companion, before anything is built:
  python main.py --enc_mode continues --fit_codebook 1024 --rvq 4 --fit_dir wavs/ --ckpt_pth CKPT
  python main.py --enc_mode continues --convert_dir in/ --t_speaker V001 --ckpt_pth CKPT --codebook ckpt_english/codebooks/K1024x4.rvq.npz
  python main.py --enc_mode continues --synth_dir idx/ --t_speaker V001 --ckpt_pth CKPT --codebook ckpt_english/codebooks/K1024x4.rvq.npz --rvq_stages 2

--rvq_train FILE.rvq.npz with --train_ae and --enc_mode continues (zs_amd.rvq_train): the autoencoder is trained through that residual
codebook -- stage 0 snaps every encoder row of a batch, stage s what stage s - 1 left over, the Decoder reads the sum of the S
codewords exactly as --convert_dir --codebook FILE.rvq.npz builds it, and its input gradient passes straight through; every stage
commits its input to its codeword (--vq_beta) and every stage's codebook follows its own input rows by the moving average of
--vq_train (--vq_decay, --vq_restart: the three options serve either flag).  The log gains loss_vq and every stage's share of
codewords used and perplexity; every checkpoint gets <checkpoint>.rvq.npz beside it, the file --codebook ... --rvq_stages s reads.
--ema, --device_data and --load_model combine with it; --vq_train, --resume, --valid_every, a multi-rank launch, every other --train*
mode and a file that is no residual codebook are refused before anything is built:
  python main.py --enc_mode continues --train_ae --load_model --rvq_train ckpt_english/codebooks/K1024x4.rvq.npz

--rvq_dropout P with --rvq_train (zs_amd.rvq_train, quantiser dropout): each step, each sample of the batch is with probability P, in
(0, 1], decoded from a number of stages drawn uniformly from 1 .. S instead of all S (drawn on the device from the step's own seed
stream, so a captured step draws anew on every replay); the stages a sample does not use neither commit its rows nor count them in
their codebooks' averages.  A model trained so has decoded rows built from 1, 2, .. stages: what --rvq_stages s speaks.  The log gains
every stage's share of active rows.  It combines with everything --rvq_train combines with, and is refused before anything is built
without --rvq_train, beside --vq_train and for a P outside (0, 1]:
  python main.py --enc_mode continues --train_ae --load_model --rvq_train ckpt_english/codebooks/K1024x4.rvq.npz --rvq_dropout 0.5

--overlap FRAMES with --synth_dir or --convert_dir (zs_amd.convert.unit_windows): a long utterance is decoded in windows of seg_len
frames that share FRAMES of them, and the shared frames are cross-faded on the device (zs_xfade_gather) instead of the pieces being
laid end to end, so the spectrogram no longer jumps every seg_len frames.  FRAMES is 0 or a multiple of 8 up to half of seg_len (64 at
the shipped settings).  The units do not change: --convert_dir encodes and writes them as without the flag and speaks them as
--synth_dir --overlap would speak the files it wrote; an utterance of at most 2 (seg_len / 8) units is one window either way.  Both
manifests gain "overlap"; a 'continues' model needs --codebook for --convert_dir --overlap, and the flag is refused without one of the
two modes, before anything is built:
  python main.py --synth_dir units/ --t_speaker V001 --ckpt_pth CKPT --overlap 32
  python main.py --convert_dir in/ --t_speaker V001,V002 --ckpt_pth CKPT --overlap 32

--segment LAMBDA with --convert_dir or --test_encode and --codebook (zs_amd.segment): the index sequence of every utterance is chosen
at once -- the sum of the frames' scores plus LAMBDA for every change of codeword is minimised exactly, on the GPU (zs_seg_viterbi)
-- instead of frame by frame, so a frame between two codewords no longer flips the symbol.  LAMBDA >= 0 is in the score's own units,
squared Euclidean distance under a vector codebook and Hamming bits under a bit codebook (the run prints which); 0 gives the files
written without the flag.  <name>.txt and <name>.idx.txt stay one line per frame, <name>.seg.txt beside them holds one line
`codeword duration` per run, and the manifest gains "segment" (segments, mean run, entropy and bits per second).  --synth_dir
--segments reads the *.seg.txt of its folder instead of the per-frame files and speaks <name>.seg.txt as <name>.wav.  A residual
codebook, K > 4096 and every other mode are refused before anything is built:
  python main.py --convert_dir in/ --t_speaker V001 --ckpt_pth CKPT --codebook ckpt_english/codebooks/K64.codebook.npz --segment 4
  python main.py --synth_dir out/convert/V001 --t_speaker V002 --ckpt_pth CKPT --codebook ckpt_english/codebooks/K64.codebook.npz --segments

--score_units DIR --abx_item FILE (zs_amd.abx, needs no checkpoint): the ABX phone discriminability of the unit files of DIR and their
bitrate.  Every token of the .item file (`file onset offset phone prev next speaker` per line, seconds) is the unit rows whose centre
lies inside it; tokens that share a context (prev, next) are compared by a dynamic time warp over frame distances (zs_abx_dtw),
Hamming for the bit unit files <name>.txt, angular for the rows of the <name>.idx.txt under --codebook, and the triplets won are
counted on the GPU (zs_abx_count).  Writes score.json (--score_out) and prints one [Score] line.  The unit files carry no time
offset (--convert_dir and preprocessing trim leading silence and do not record by how much): --abx_offsets gives it per file.
  python main.py --score_units out/convert/V001 --abx_item english.item --abx_task within,across
  python main.py --score_units out/convert/V001 --abx_item english.item --codebook ckpt_english/codebooks/K64.vq.npz

Multi-GPU training: `python -m torch.distributed.run --nproc-per-node N main.py --train_ae ...` (one
process per GPU; gradients are averaged with RCCL).  Modes outside the stage-1 autoencoder path
(--train_al, --train_t, --encode, --test_asr) are not part of this build and exit with a clear error.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

OUT_OF_SCOPE = ['train_al', 'train_t', 'test_asr', 'encode']


def _gl_iters(text):
    n = int(text)
    if n < 0:
        raise argparse.ArgumentTypeError('--gl_iters must be a non-negative integer (got %s)' % text)
    return n


def _gl_momentum(text):
    try:
        a = float(text)
    except ValueError:
        raise argparse.ArgumentTypeError('--gl_momentum must be a number in [0, 1) (got %s)' % text)
    if not 0.0 <= a < 1.0:                    # NaN fails too
        raise argparse.ArgumentTypeError('--gl_momentum must be in [0, 1) (got %s)' % text)
    return a


def _out_sr(text):
    try:
        n = int(text)
    except ValueError:
        raise argparse.ArgumentTypeError('--out_sr must be a positive integer (got %s)' % text)
    if n <= 0 or n > 32 * 16000 or 32 * n < 16000:
        raise argparse.ArgumentTypeError('--out_sr must be a positive integer with out_sr / 16000 within [1/32, 32] (got %s)' % text)
    return n


def _ema(text):
    try:
        d = float(text)
    except ValueError:
        raise argparse.ArgumentTypeError('--ema must be a number in [0, 1) (got %s)' % text)
    if not 0.0 <= d < 1.0:                    # NaN fails too
        raise argparse.ArgumentTypeError('--ema must be in [0, 1) (got %s)' % text)
    return d


def _codebook_k(text):
    try:
        k = int(text)
    except ValueError:
        raise argparse.ArgumentTypeError('--fit_codebook must be an integer in [1, 65536] (got %s)' % text)
    if not 1 <= k <= 65536:
        raise argparse.ArgumentTypeError('--fit_codebook must be in [1, 65536] (got %s)' % text)
    return k


def _codebook_iters(text):
    try:
        n = int(text)
    except ValueError:
        raise argparse.ArgumentTypeError('--codebook_iters must be a positive integer (got %s)' % text)
    if n < 1:
        raise argparse.ArgumentTypeError('--codebook_iters must be >= 1 (got %s)' % text)
    return n


def _rvq(text):
    try:
        s = int(text)
    except ValueError:
        raise argparse.ArgumentTypeError('--rvq must be an integer in [2, 8] (got %s)' % text)
    if not 2 <= s <= 8:
        raise argparse.ArgumentTypeError('--rvq must be in [2, 8] (got %s)' % text)
    return s


def _rvq_stages(text):
    try:
        s = int(text)
    except ValueError:
        raise argparse.ArgumentTypeError('--rvq_stages must be an integer in [1, 8] (got %s)' % text)
    if not 1 <= s <= 8:
        raise argparse.ArgumentTypeError('--rvq_stages must be in [1, 8] (got %s)' % text)
    return s


VALID_BATCHES = 8
CODEBOOK_ITERS = 20


def build_parser():
    p = argparse.ArgumentParser(description='zerospeech_project (MI355X autoencoder hot path)')
    for flag in ['preprocess', 'train', 'train_ae', 'train_p', 'train_tgat', 'train_c', 'test', 'cross_test', 'test_encode', 'test_single',
                 'test_classify', 'load_model', 'enc_only', 'remake', 'synthetic'] + OUT_OF_SCOPE:
        p.add_argument('--' + flag, default=False, action='store_true')
    p.add_argument('--device_data', default=False, action='store_true',
                   help='every --train* mode: hold the training set in GPU memory and gather each batch on the device '
                        '(zs_amd.pool; size limit ZS_POOL_MAX_GB); default: the host DataLoader')
    p.add_argument('--resume', default=False, action='store_true',
                   help='with one of --train_ae / --train_p / --train_tgat / --train_c: write a train-state file beside every '
                        'checkpoint and continue from the newest one in --ckpt_dir (from iteration 0 when there is none)')
    p.add_argument('--flag', type=str, default='train')
    p.add_argument('--g_mode', default='set_from_hps',
                   choices=['naive', 'targeted', 'targeted_residual', 'enhanced', 'spectrogram', 'tacotron', 'set_from_hps'])
    p.add_argument('--enc_mode', default='set_from_hps',
                   choices=['continues', 'one_hot', 'binary', 'multilabel_binary', 'gumbel_t', 'set_from_hps'])
    p.add_argument('--dataset', choices=['english', 'surprise'], default='english')
    p.add_argument('--dtype', choices=['fp32', 'bf16'], default=os.environ.get('ZS_DTYPE', 'bf16'))
    p.add_argument('--source_path', type=str, default='./data/english/train/unit/')
    p.add_argument('--target_path', type=str, default='./data/english/train/voice/')
    p.add_argument('--test_path', type=str, default='./data/english/test/')
    p.add_argument('--synthesis_list', type=str, default='./data/english/synthesis.txt')
    p.add_argument('--dataset_path', type=str, default='./data/dataset_english.hdf5')
    p.add_argument('--index_path', type=str, default='./data/index_english.json')
    p.add_argument('--index_source_path', type=str, default='./data/index_english_source.json')
    p.add_argument('--index_target_path', type=str, default='./data/index_english_target.json')
    p.add_argument('--speaker2id_path', type=str, default='./data/speaker2id_english.json')
    p.add_argument('--hps_path', type=str, default='./hps/zerospeech_english.json')
    p.add_argument('--ckpt_dir', type=str, default='./ckpt_english')
    p.add_argument('--result_dir', type=str, default='./result')
    p.add_argument('--sub_result_dir', type=str, default='./english/')
    p.add_argument('--model_name', type=str, default='model.pth')
    p.add_argument('--load_train_model_name', type=str, default='model.pth-ae-424000')
    p.add_argument('--load_test_model_name', type=str, default='model.pth-s2-150000')
    p.add_argument('--ckpt_pth', type=str, default=None)
    p.add_argument('--load_tclf_model_name', type=str, default=None)     # main.py:79: a path, used as given
    p.add_argument('--s_speaker', type=str, default='S015')
    p.add_argument('--t_speaker', type=str, default='V002', help='target speaker; with --convert_dir / --synth_dir a comma-separated list')
    p.add_argument('--convert_dir', type=str, default=None, metavar='DIR',
                   help='convert every *.wav of DIR (any PCM / float format, any rate) to each --t_speaker, on the GPU from the '
                        'samples to the waveform; outputs under {result_dir}/{sub_result_dir}/convert/')
    p.add_argument('--synth_dir', type=str, default=None, metavar='DIR',
                   help='synthesise every *.txt of DIR (unit files: one line of 0 / 1 per encoded frame) in the voice of each '
                        '--t_speaker; outputs under {result_dir}/{sub_result_dir}/synth/')
    p.add_argument('--gl_iters', type=_gl_iters, default=None, help='Griffin-Lim iterations (hp.n_iter); default: leave hp as it is')
    p.add_argument('--gl_momentum', type=_gl_momentum, default=None,
                   help='fast Griffin-Lim momentum in [0, 1) (hp.gl_momentum); default: leave hp as it is')
    p.add_argument('--ema', type=_ema, default=None, metavar='D',
                   help='every --train* mode: keep an exponential moving average of the weights with decay D in [0, 1), updated in '
                        'the Adam kernels; checkpoints gain <net>_ema entries; default: none')
    p.add_argument('--use_ema', default=False, action='store_true',
                   help='load the averaged weights (<net>_ema) of the checkpoint: every --test* mode, --cross_test, --convert_dir, --synth_dir, and '
                        'training with --load_model')
    p.add_argument('--valid_every', type=int, default=None, metavar='N',
                   help='--train_ae / --train: validate the autoencoder on a held-out set after every N-th pretrain_AE iteration and '
                        'the last; records in <ckpt_dir>/valid.jsonl, best checkpoint <model_name>-ae-best (a run without --resume starts both '
                        'anew: an existing valid.jsonl in --ckpt_dir is emptied, -ae-best overwritten); default: never')
    p.add_argument('--valid_batches', type=int, default=None, metavar='M',
                   help='with --valid_every: batches of hps.batch_size segments in the validation set (default %d)' % VALID_BATCHES)
    p.add_argument('--valid_index_path', type=str, default=None,
                   help='with --valid_every: index JSON of the validation set over --dataset_path (its first M * batch_size entries)')
    p.add_argument('--valid_holdout', type=int, default=None, metavar='K',
                   help='with --valid_every: hold every K-th utterance (K >= 2) of --index_path out of training as the validation set')
    p.add_argument('--valid_flag', type=str, default=None,
                   help="with --valid_index_path: the group of --dataset_path its entries lie in (default 'train')")
    p.add_argument('--adapt_voice', type=str, default=None, metavar='NAME',
                   help='enrol a new target voice NAME from the *.wav of --adapt_dir: fit its five Decoder embedding rows with every '
                        'other weight frozen and write {voice_dir}/NAME.voice.npz')
    p.add_argument('--adapt_dir', type=str, default=None, metavar='DIR', help='with --adapt_voice: the folder of its utterances')
    p.add_argument('--adapt_iters', type=int, default=None, metavar='N', help='with --adapt_voice: iterations (default 500)')
    p.add_argument('--adapt_init', type=str, default=None, metavar='SPEAKER',
                   help="with --adapt_voice: start from this speaker's rows (default: the mean of each table's rows)")
    p.add_argument('--adapt_lr', type=float, default=None, metavar='LR', help='with --adapt_voice: learning rate (default hps.lr)')
    p.add_argument('--voice_dir', type=str, default=None, metavar='DIR', help='with --adapt_voice: where the voice file goes (default {ckpt_dir}/voices)')
    p.add_argument('--voice', action='append', default=None, metavar='NAME=FILE',
                   help='with --convert_dir / --synth_dir and --enc_only: register the voice file FILE as target speaker NAME (repeatable)')
    p.add_argument('--fit_codebook', type=_codebook_k, default=None, metavar='K',
                   help='fit a codebook of K codewords to the units of --fit_dir on the GPU and write it to --codebook_out: k-modes in '
                        "Hamming distance, or for enc_mode 'continues' k-means over the encoder's vectors (a vector codebook)")
    p.add_argument('--fit_dir', type=str, default=None, metavar='DIR',
                   help='with --fit_codebook: the folder of *.wav (encoded as --convert_dir reads them) and *.txt unit files')
    p.add_argument('--codebook_out', type=str, default=None, metavar='FILE',
                   help="with --fit_codebook: where the codebook goes (default {ckpt_dir}/codebooks/K<K>.codebook.npz, K<K>.vq.npz for "
                        "enc_mode 'continues')")
    p.add_argument('--codebook_iters', type=_codebook_iters, default=None, metavar='N',
                   help='with --fit_codebook: k-modes iterations at most (default %d)' % CODEBOOK_ITERS)
    p.add_argument('--codebook_seed', type=int, default=None, metavar='S', help='with --fit_codebook: seed of the starting codewords (default 0)')
    p.add_argument('--codebook', type=str, default=None, metavar='FILE',
                   help='with --convert_dir / --synth_dir / --test_encode: snap every unit to its nearest codeword of this codebook; a '
                        "vector codebook (FILE.vq.npz, enc_mode 'continues') writes <name>.idx.txt index files, and --synth_dir reads them")
    p.add_argument('--rvq', type=_rvq, default=None, metavar='S',
                   help="with --fit_codebook and enc_mode 'continues': fit a residual codebook of S stages of K codewords each, S in "
                        '[2, 8] (default file {ckpt_dir}/codebooks/K<K>x<S>.rvq.npz)')
    p.add_argument('--rvq_stages', type=_rvq_stages, default=None, metavar='s',
                   help='with --codebook FILE.rvq.npz: use the first s stages of the residual codebook (default: all of them for '
                        "--convert_dir and --test_encode, a unit file's own columns for --synth_dir)")
    p.add_argument('--vq_train', type=str, default=None, metavar='FILE',
                   help="with --train_ae and enc_mode 'continues': train through the vector codebook FILE.vq.npz (straight-through "
                        'quantiser, commitment term, codebook by exponential moving average); every checkpoint gets a '
                        '<checkpoint>.vq.npz beside it, the file --codebook reads')
    p.add_argument('--rvq_train', type=str, default=None, metavar='FILE',
                   help="with --train_ae and enc_mode 'continues': train through the residual codebook FILE.rvq.npz (every stage a "
                        'straight-through quantiser of what the stage before left over, with its own commitment term and moving '
                        'average); every checkpoint gets a <checkpoint>.rvq.npz beside it, the file --codebook and --rvq_stages read')
    p.add_argument('--vq_beta', type=float, default=None, metavar='B',
                   help='with --vq_train or --rvq_train: commitment weight in (0, 10] (default 0.25)')
    p.add_argument('--vq_decay', type=float, default=None, metavar='D',
                   help="with --vq_train or --rvq_train: decay of the codebook's moving average in [0, 1) (default 0.99)")
    p.add_argument('--vq_restart', type=float, default=None, metavar='T',
                   help='with --vq_train or --rvq_train: a codeword that took no row of the batch and whose averaged count fell below '
                        "T, in (0, 1), is put back onto one of the rows its stage quantised (default: dead codewords stay where they are)")
    p.add_argument('--rvq_dropout', type=float, default=None, metavar='P',
                   help='with --rvq_train: quantiser dropout -- with probability P in (0, 1] a sample of the batch is decoded from a number '
                        'of stages drawn uniformly from 1 .. S instead of all S (default: every sample from all S)')
    p.add_argument('--overlap', type=int, default=None, metavar='FRAMES',
                   help='with --synth_dir / --convert_dir: decode in windows that share FRAMES spectrogram frames and cross-fade them '
                        '(0, or a multiple of 8 up to 8 * ((seg_len // 8) // 2)); the units do not change; default: pieces laid end to end')
    p.add_argument('--segment', type=float, default=None, metavar='LAMBDA',
                   help='with --convert_dir / --test_encode and --codebook: choose the codeword sequence of every utterance at once, '
                        "LAMBDA >= 0 per change of codeword in the score's own units (squared Euclidean distance or Hamming bits); "
                        'writes <name>.seg.txt beside the per-frame unit files; default: every frame alone')
    p.add_argument('--segments', action='store_true',
                   help='with --synth_dir and --codebook: read the *.seg.txt run files of the folder instead of its per-frame unit files')
    p.add_argument('--score_units', type=str, default=None, metavar='DIR',
                   help='score the unit files of DIR (no checkpoint needed): ABX error by batched DTW on the GPU against --abx_item, and '
                        'the bitrate; <name>.txt bit unit files, or <name>.idx.txt with --codebook; writes score.json')
    p.add_argument('--abx_item', type=str, default=None, metavar='FILE',
                   help='with --score_units: the ABX .item file (a # header, then `file onset offset phone prev next speaker`, seconds)')
    p.add_argument('--abx_task', type=str, default=None, metavar='TASKS', help='with --score_units: within, across or within,across (default both)')
    p.add_argument('--abx_metric', choices=['hamming', 'angular'], default=None,
                   help='with --score_units: the frame distance (default hamming for bit units, angular under a vector or residual codebook)')
    p.add_argument('--abx_offsets', type=str, default=None, metavar='FILE.json',
                   help='with --score_units: a json object of seconds to add per file stem; --convert_dir and preprocessing trim leading '
                        'silence and do not record by how much, so a trimmed file needs its offset from here')
    p.add_argument('--score_out', type=str, default=None, metavar='FILE', help='with --score_units: where score.json goes (default DIR/score.json)')
    p.add_argument('--out_sr', type=_out_sr, default=None,
                   help='sample rate of the wavs --test / --cross_test / --test_single write (hp.out_sr); default: 16000')
    return p


RESUMABLE = ['train_ae', 'train_p', 'train_tgat', 'train_c']


def check_resume(args):
    """--resume continues ONE stage from its own newest checkpoint: refuse, before anything is built, the chained --train, more
    than one stage flag, and --load_model (the weights come from the checkpoint that is resumed)."""
    if not args.resume:
        return
    if args.train:
        raise ValueError('--resume continues one stage: use it with --train_ae, --train_p, --train_tgat or --train_c, not with the '
                         'chained --train')
    stages = [f for f in RESUMABLE if getattr(args, f)]
    if len(stages) != 1:
        raise ValueError('--resume needs exactly one of %s (got %s)' % (', '.join('--' + f for f in RESUMABLE),
                                                                        ', '.join('--' + f for f in stages) or 'none'))
    if args.load_model:
        raise ValueError('--resume loads the newest checkpoint of its stage itself: it cannot be combined with --load_model')


TRAIN_MODES = ['train', 'train_ae', 'train_p', 'train_tgat', 'train_c']


LOADING_MODES = ['test', 'cross_test', 'test_encode', 'test_single', 'test_classify']


def check_ema(args):
    """--ema averages the weights a training run updates, --use_ema chooses what a checkpoint is loaded from: each is refused,
    before anything is built, where it would have no effect -- --ema without a --train* mode, --use_ema without a mode that loads
    a checkpoint (a --test* mode, --cross_test, --convert_dir, --synth_dir, or a --train* mode with --load_model)."""
    training = any(getattr(args, f) for f in TRAIN_MODES)
    if args.ema is not None and not training:
        raise ValueError('--ema needs a training mode (%s)' % ', '.join('--' + f for f in TRAIN_MODES))
    loads = any(getattr(args, f) for f in LOADING_MODES) or args.convert_dir is not None or args.synth_dir is not None or \
        (training and args.load_model) or getattr(args, 'adapt_voice', None) is not None or \
        getattr(args, 'fit_codebook', None) is not None
    if args.use_ema and not loads:
        raise ValueError('--use_ema needs a mode that loads a checkpoint: %s, --convert_dir, or a training mode with --load_model'
                         % ', '.join('--' + f for f in LOADING_MODES))


def voice_files(args):
    """--voice NAME=FILE ... as {name: file}, in order; ValueError for an entry of another form or a name given twice."""
    specs = getattr(args, 'voice', None) or []
    if not specs:
        return {}
    from zs_amd.voice import parse_voices
    return parse_voices(specs)


def check_voice(args, speaker2id=None):
    """--adapt_voice and --voice are refused, before anything is built, where they cannot do what they say: --adapt_voice without
    --adapt_dir, with a --train* mode, with any mode that converts or tests (a command adapts OR uses a voice) or under a multi-rank launch; --voice without --convert_dir / --synth_dir or without --enc_only
    (voices convert through the autoencoder alone); a name that is a speaker of speaker2id already or is given twice; an --adapt_init
    that is no such speaker; --adapt_iters < 1; and enc_mode 'continues', which has no units to cache (checked once --enc_mode is
    known: argument_runner calls this again after reading hps).  speaker2id: the table, read from --speaker2id_path when None
    and the file exists."""
    adapt, voices = getattr(args, 'adapt_voice', None), voice_files(args)
    if adapt is None:
        for flag in ('adapt_dir', 'adapt_iters', 'adapt_init', 'adapt_lr', 'voice_dir'):
            if getattr(args, flag, None) is not None:
                raise ValueError('--%s needs --adapt_voice' % flag)
    if adapt is None and not voices:
        return
    if speaker2id is None and os.path.exists(args.speaker2id_path):
        import json
        with open(args.speaker2id_path, 'r') as f:
            speaker2id = json.load(f)
    speaker2id = speaker2id or {}
    if adapt is not None:
        if not adapt.strip() or adapt != adapt.strip() or any(ch in adapt for ch in ',=/\\'):
            raise ValueError("--adapt_voice needs a name without ',', '=', '/' or surrounding blanks (got %r)" % adapt)
        if args.adapt_dir is None:
            raise ValueError('--adapt_voice needs --adapt_dir DIR, the folder of the voice\'s utterances')
        modes = [f for f in TRAIN_MODES if getattr(args, f)]
        if modes:
            raise ValueError('--adapt_voice fits a voice to a finished checkpoint: it cannot be combined with --%s' % modes[0])
        if int(os.environ.get('WORLD_SIZE', '1')) > 1:
            raise ValueError('--adapt_voice runs on one GPU: start it without a multi-rank launcher (WORLD_SIZE = %s)' % os.environ['WORLD_SIZE'])
        others = [f for f in LOADING_MODES if getattr(args, f)] + [f for f in ('convert_dir', 'synth_dir') if getattr(args, f) is not None]
        if voices or others:
            raise ValueError('--adapt_voice writes a voice and does nothing else: run --%s as a command of its own'
                             % (others[0] if others else 'voice'))
        if adapt in speaker2id:
            raise ValueError('--adapt_voice %r is a speaker of %s already' % (adapt, args.speaker2id_path))
        if args.adapt_init is not None and args.adapt_init not in speaker2id:
            raise ValueError('--adapt_init %r is not in %s' % (args.adapt_init, args.speaker2id_path))
        if args.adapt_iters is not None and args.adapt_iters < 1:
            raise ValueError('--adapt_iters must be >= 1 (got %d)' % args.adapt_iters)
        if args.adapt_lr is not None and not args.adapt_lr > 0.0:
            raise ValueError('--adapt_lr must be > 0 (got %r)' % args.adapt_lr)
    if voices:
        if args.convert_dir is None and args.synth_dir is None:
            raise ValueError('--voice needs --convert_dir or --synth_dir')
        if not args.enc_only:
            raise ValueError('--voice needs --enc_only: voices convert through the autoencoder alone (the stage-2 generator has rows '
                             'for its trained target speakers only)')
        for name in voices:
            if name in speaker2id:
                raise ValueError('--voice %r is a speaker of %s already' % (name, args.speaker2id_path))
    if args.enc_mode == 'continues':
        raise ValueError("enc_mode 'continues' has no units to cache: voices need a discrete encoder mode")


def check_codebook(parser, args):
    """The codebook flags that cannot do what they say are argparse errors: --fit_codebook without --fit_dir (and the reverse), its
    options without it, --fit_codebook beside a --train* mode, and --codebook without a mode that takes it."""
    if args.fit_codebook is not None and args.fit_dir is None:
        parser.error('--fit_codebook needs --fit_dir DIR, the folder whose units are clustered')
    if args.fit_codebook is None:
        for flag in ('fit_dir', 'codebook_out', 'codebook_iters', 'codebook_seed'):
            if getattr(args, flag) is not None:
                parser.error('--%s needs --fit_codebook' % flag)
    elif any(getattr(args, f) for f in TRAIN_MODES):
        parser.error('--fit_codebook fits a codebook to a finished checkpoint: it cannot be combined with a --train* mode')
    if args.codebook is not None and not (args.convert_dir is not None or args.synth_dir is not None or args.test_encode or
                                          getattr(args, 'score_units', None) is not None):
        parser.error('--codebook needs --convert_dir, --synth_dir or --test_encode (or --score_units)')
    if args.codebook is not None and args.fit_codebook is not None:
        parser.error('--codebook uses a codebook and --fit_codebook writes one: run them as two commands')


def check_rvq(args, enc_mode=None):
    """--rvq and --rvq_stages are refused, before anything is built, where they cannot do what they say: --rvq without --fit_codebook,
    --rvq_stages without --codebook; and, once enc_mode is known (argument_runner calls this again after reading hps), --rvq for an
    enc_mode other than 'continues', --rvq_stages for a file that is no residual codebook or has fewer stages, and a residual
    codebook for an enc_mode other than 'continues' (the file's fields are read here)."""
    rvq, stages = getattr(args, 'rvq', None), getattr(args, 'rvq_stages', None)
    if rvq is not None and getattr(args, 'fit_codebook', None) is None:
        raise ValueError('--rvq needs --fit_codebook K: it sets the stages of the residual codebook that is fitted')
    if stages is not None and getattr(args, 'codebook', None) is None:
        raise ValueError('--rvq_stages needs --codebook FILE.rvq.npz: it chooses how many stages of that residual codebook are used')
    if enc_mode is None:
        return
    if rvq is not None and enc_mode != 'continues':
        raise ValueError("--rvq fits a residual codebook, which serves enc_mode 'continues': this model's enc_mode is %r" % enc_mode)
    path = getattr(args, 'codebook', None)
    if path is None or (stages is None and not path.endswith('.rvq.npz')):      # (every other file is read where it always was)
        return
    from zs_amd.codebook import read_npz
    d = read_npz(path)
    residual = 'kind' in d and d['kind'].shape == () and str(d['kind']) == 'residual'
    if residual:
        from zs_amd.rvq import ResidualCodebook
        ResidualCodebook.check_mode(enc_mode, "--codebook %s is a residual codebook (kind 'residual'), which serves enc_mode 'continues'" % path)
    if stages is not None:
        if not residual:
            raise ValueError('--rvq_stages needs a residual codebook (FILE.rvq.npz): %s is none' % path)
        if 'S' in d and d['S'].shape == () and d['S'].dtype.kind in 'iu' and stages > int(d['S']):
            raise ValueError('--rvq_stages %d: %s has S = %d stages' % (stages, path, int(d['S'])))


def check_vq_train(args, enc_mode=None, c_in=None):
    """--vq_train, --vq_beta, --vq_decay and --vq_restart are refused, before anything is built, where they cannot do what they say
    (zs_amd.vq_train.check_vq_train): without --train_ae or beside another --train* mode, under a multi-rank launch, with --resume
    or --valid_every, the two options without --vq_train or out of range; and, once enc_mode is known (argument_runner calls
    this again after reading hps), an enc_mode other than 'continues', a bit codebook or a width other than the Decoder's c_in.
    Returns the loaded codebook on that second call (None without --vq_train)."""
    from zs_amd.vq_train import check_vq_train as check
    return check(args, enc_mode, c_in)


def check_rvq_train(args, enc_mode=None, c_in=None):
    """--rvq_train is refused, before anything is built and naming the flag, where it cannot do what it says
    (zs_amd.rvq_train.check_rvq_train): beside --vq_train, without --train_ae or beside another --train* mode, under a multi-rank
    launch, with --resume or --valid_every, its options out of range (--rvq_dropout too: without --rvq_train, beside --vq_train or with
    a P outside (0, 1]); and, once enc_mode is known (argument_runner calls this again
    after reading hps), an enc_mode other than 'continues', a file that is no residual codebook or a width other than the Decoder's
    c_in.  Returns the loaded codebook on that second call (None without --rvq_train)."""
    from zs_amd.rvq_train import check_rvq_train as check
    return check(args, enc_mode, c_in)


def check_overlap(args, seg_len=None, enc_mode=None):
    """--overlap is refused, before anything is built, where it cannot do what it says: without --synth_dir or --convert_dir; and,
    once hps is read (argument_runner calls this again with its seg_len and the enc_mode), for a value outside the window rule of
    that seg_len (zs_amd.convert.check_overlap_value) and with --convert_dir on a 'continues' model without --codebook, which has
    no units to speak from."""
    overlap = getattr(args, 'overlap', None)
    if overlap is None:
        return
    if args.convert_dir is None and args.synth_dir is None:
        raise ValueError('--overlap needs --synth_dir or --convert_dir: it sets how their decode windows are joined')
    if seg_len is None:
        return
    from zs_amd.convert import check_overlap_value
    try:
        check_overlap_value(overlap, seg_len)
    except ValueError as e:
        raise ValueError('--overlap: %s' % e)
    if overlap and args.convert_dir is not None and enc_mode == 'continues' and getattr(args, 'codebook', None) is None:
        raise ValueError("--overlap with --convert_dir speaks the units it writes: enc_mode 'continues' has none without --codebook")


SEGMENT_MODES = ('convert_dir', 'test_encode')
NOT_SEGMENT_MODES = ('synth_dir', 'test', 'cross_test', 'test_single', 'test_classify', 'fit_codebook', 'adapt_voice', 'preprocess')


def _residual_file(path):
    """Whether the codebook file holds a residual codebook, by its fields (a file that cannot be read is reported where it is loaded)."""
    from zs_amd.codebook import read_npz
    try:
        d = read_npz(path)
    except ValueError:
        return False
    return 'kind' in d and d['kind'].shape == () and str(d['kind']) == 'residual'


def check_segment(args, enc_mode=None):
    """--segment and --segments are refused, before anything is built, where they cannot do what they say: --segment without
    --convert_dir or --test_encode, beside any other mode, without --codebook, with --rvq_stages or a value that is no finite number
    >= 0; --segments without --synth_dir or --codebook, or beside --segment; and either with a residual codebook (by the file's
    name, and by its fields once hps is read: argument_runner calls this again)."""
    lam, runs_in = getattr(args, 'segment', None), getattr(args, 'segments', False)
    if lam is None and not runs_in:
        return
    flag = '--segment' if lam is not None else '--segments'
    if lam is not None:
        from zs_amd.segment import check_lambda
        check_lambda(lam, '--segment')
        if runs_in:
            raise ValueError('--segment writes run files and --segments reads them: run them as two commands')
        if not (args.convert_dir is not None or args.test_encode):
            raise ValueError('--segment needs --convert_dir or --test_encode: it chooses the units they write')
        other = [m for m in NOT_SEGMENT_MODES + tuple(TRAIN_MODES) if getattr(args, m, None) not in (None, False)]
        if other:
            raise ValueError('--segment serves --convert_dir and --test_encode alone: it cannot be combined with --%s' % other[0])
    elif args.synth_dir is None:
        raise ValueError('--segments needs --synth_dir: it makes it read the *.seg.txt run files of its folder')
    if getattr(args, 'codebook', None) is None:
        raise ValueError('%s needs --codebook FILE: the runs are sequences of its codewords' % flag)
    if getattr(args, 'rvq_stages', None) is not None or args.codebook.endswith('.rvq.npz') or (enc_mode is not None and _residual_file(args.codebook)):
        raise ValueError('%s does not segment the stages of a residual codebook: use a bit or a vector codebook' % flag)


SCORE_FLAGS = ('abx_item', 'abx_task', 'abx_metric', 'abx_offsets', 'score_out')
NOT_SCORE_MODES = ('convert_dir', 'synth_dir', 'test', 'cross_test', 'test_single', 'test_encode', 'test_classify', 'fit_codebook',
                   'adapt_voice', 'preprocess', 'segment', 'segments', 'rvq_stages', 'overlap')


def check_score(args):
    """--score_units and its options are refused, before anything is read, where they cannot do what they say: an option without
    --score_units, --score_units without --abx_item, beside any other mode, or with an --abx_task other than within / across."""
    if getattr(args, 'score_units', None) is None:
        for flag in SCORE_FLAGS:
            if getattr(args, flag, None) is not None:
                raise ValueError('--%s needs --score_units DIR' % flag)
        return
    if args.abx_item is None:
        raise ValueError('--score_units needs --abx_item FILE: the tokens to compare')
    other = [m for m in NOT_SCORE_MODES + tuple(TRAIN_MODES) if getattr(args, m, None) not in (None, False)]
    if other:
        raise ValueError('--score_units scores unit files that are already written: it cannot be combined with --%s' % other[0])
    if args.abx_task is not None:
        from zs_amd.abx import check_tasks
        check_tasks(args.abx_task)


def convert_targets(args):
    """--convert_dir and --synth_dir take --t_speaker as a comma-separated list of distinct names (--test_single keeps the single name): the
    list, refused before anything is built when it names no speaker or one twice."""
    names = [t.strip() for t in args.t_speaker.split(',')]
    if not all(names):
        raise ValueError('--convert_dir needs --t_speaker NAME[,NAME...] (got %r)' % args.t_speaker)
    if len(set(names)) != len(names):
        raise ValueError('--t_speaker names a speaker twice (got %r)' % args.t_speaker)
    return names


def argument_runner(argv=None):
    from zs_amd.hps import Hps, hp
    parser = build_parser()
    args = parser.parse_args(argv)
    check_codebook(parser, args)
    check_resume(args)
    check_ema(args)
    check_voice(args)
    from zs_amd.validation import check_flags
    check_flags(args)
    check_vq_train(args)
    check_rvq_train(args)
    check_rvq(args)
    check_overlap(args)
    check_segment(args)
    check_score(args)
    if args.score_units is not None:          # needs no checkpoint and no hps: nothing below applies
        return args, None
    args.t_speakers =convert_targets(args) if (args.convert_dir is not None or args.synth_dir is not None) else None
    if args.dataset == 'surprise':            # main.py:83-88: english -> surprise in every default path
        for action in parser._actions:
            if isinstance(action.default, str) and 'english' in action.default and \
                    ('path' in action.dest or action.dest in ('synthesis_list', 'sub_result_dir', 'ckpt_dir')):
                action.default = action.default.replace('english', 'surprise')
        args = parser.parse_args(argv)
    print('[Runner] - Dataset: ', args.dataset)
    if args.gl_iters is not None:             # the vocoder of --test / --cross_test / --test_single reads hp
        hp.n_iter = args.gl_iters
    if args.gl_momentum is not None:
        hp.gl_momentum = args.gl_momentum
    if args.out_sr is not None:
        hp.out_sr = args.out_sr
    hps = Hps(args.hps_path).get_tuple()
    if args.g_mode == 'set_from_hps':
        args.g_mode = hps.g_mode
    if args.enc_mode == 'set_from_hps':
        args.enc_mode = hps.enc_mode
    check_voice(args)                         # again, now that enc_mode is known
    args.vq_codebook = check_vq_train(args, args.enc_mode, hps.enc_size)      # (the file is read here: a bit codebook or another width)
    if args.vq_codebook is None:              # --rvq_train: the same slot, a residual codebook in it (the Trainer picks by its kind)
        args.vq_codebook = check_rvq_train(args, args.enc_mode, hps.enc_size)
    check_rvq(args, args.enc_mode)            # again, now that enc_mode is known (a residual codebook's fields are read here)
    check_overlap(args, hps.seg_len, args.enc_mode)      # again, now that seg_len and enc_mode are known
    check_segment(args, args.enc_mode)        # again: a residual codebook is told by its fields
    print('[Runner] - Generation mode: ', 'autoencoder only' if args.enc_only else 'with generator')
    print('[Runner] - Generator mode: ', args.g_mode)
    print('[Runner] - Encoder mode: ', args.enc_mode)
    print('[Runner] - Encoding dim: ', hps.enc_size)
    return args, hps


def training_sets(args, hps, world=1):
    """(dataset, sourceset, targetset, valid) of a --train* run: the three sets the loaders are built over and the ValidConfig of
    --valid_every (None without it).  --valid_holdout takes every K-th utterance of --index_path out of `dataset` (the stage-2
    sets are not touched); the validation set is read, and checked (ValueError), here."""
    from zs_amd.dataloader import Dataset, SyntheticDataset
    n_syn = max(4 * hps.batch_size * world, 64)
    validset = None
    if args.synthetic:
        dataset = SyntheticDataset(n_syn, seg_len=hps.seg_len, n_speakers=hps.n_speakers)
        sourceset = SyntheticDataset(n_syn, seg_len=hps.seg_len, n_speakers=max(1, hps.n_speakers - hps.n_target_speakers), seed=1)
        targetset = SyntheticDataset(n_syn, seg_len=hps.seg_len, n_speakers=hps.n_target_speakers, seed=2,
                                     speaker_offset=hps.n_speakers - hps.n_target_speakers)
    else:
        dataset = Dataset(args.dataset_path, args.index_path, seg_len=hps.seg_len)
        sourceset = Dataset(args.dataset_path, args.index_source_path, seg_len=hps.seg_len)
        targetset = Dataset(args.dataset_path, args.index_target_path, seg_len=hps.seg_len)
        if args.valid_every is not None and args.valid_holdout is not None:      # every K-th utterance leaves the training set
            from zs_amd import validation
            kept, held = validation.holdout_split(dataset.indexes, args.valid_holdout)
            dataset = Dataset(args.dataset_path, args.index_path, seg_len=hps.seg_len, indexes=kept)
            validset = Dataset(args.dataset_path, args.index_path, seg_len=hps.seg_len, indexes=held)
    valid = None
    if args.valid_every is not None:
        from zs_amd.validation import ValidConfig, ValidSet
        M = args.valid_batches if args.valid_batches is not None else VALID_BATCHES
        if args.valid_index_path is not None:
            validset = Dataset(args.dataset_path, args.valid_index_path, dset=args.valid_flag or 'train', seg_len=hps.seg_len)
        elif validset is None:
            validset = SyntheticDataset(M * hps.batch_size, seg_len=hps.seg_len, n_speakers=hps.n_speakers, seed=3)
        valid = ValidConfig(args.valid_every, M, ValidSet.from_dataset(validset, M, hps.batch_size, hps.n_speakers), args.valid_holdout)
    return dataset, sourceset, targetset, valid


def main(argv=None):
    import zs_amd  # noqa: F401
    args, hps = argument_runner(argv)
    if args.score_units is not None:                      # not in the reference: ABX error and bitrate of a folder of unit files (zs_amd.abx)
        from zs_amd import abx
        cb = abx.load_codebook(args.codebook) if args.codebook is not None else None
        abx.score_units(args.score_units, args.abx_item, tasks=(args.abx_task or 'within,across'), metric=args.abx_metric, codebook=cb,
                        offsets=(abx.read_offsets(args.abx_offsets) if args.abx_offsets is not None else None), out_path=args.score_out)
        return
    bad = [f for f in OUT_OF_SCOPE if getattr(args, f)]
    if bad:
        raise NotImplementedError('--%s is outside the stage-1 autoencoder hot path this build covers' % bad[0])
    from zs_amd import parallel
    from zs_amd.convert import convert_dir, cross_test, get_trainer, synth_dir, target_classify, test_encode, test_from_list, test_single
    from zs_amd.dataloader import DataLoader
    from zs_amd.trainer import Trainer

    if args.preprocess:                                   # main.py:113-126
        from zs_amd.preprocess import preprocess
        preprocess(args.source_path, args.target_path, args.test_path, args.dataset_path, args.index_path, args.index_source_path,
                   args.index_target_path, args.speaker2id_path, seg_len=hps.seg_len, n_samples=hps.n_samples, dset=args.flag,
                   remake=args.remake)

    if args.train or args.train_ae or args.train_p or args.train_tgat or args.train_c:   # main.py:129-171
        rank, world, _ = parallel.init_from_env()
        dataset, sourceset, targetset, valid = training_sets(args, hps, world)   # (ValueError of the validation set: before the trainer and any pool)
        if args.device_data:
            # the sets the chosen modes read, uploaded once into one pool (index files over one store share their utterances)
            import torch
            from zs_amd.pool import DevicePool, PoolLoader
            stage1, stage2 = args.train or args.train_ae or args.train_c, args.train or args.train_p or args.train_tgat
            used = ([dataset] if stage1 else []) + ([sourceset, targetset] if stage2 else [])
            pool = DevicePool(used, torch.device('cuda', int(os.environ.get('LOCAL_RANK', '0'))))
            mk = lambda ds: PoolLoader(pool, ds, hps.batch_size, rank=rank, world=world) if any(ds is u for u in used) else None
        else:
            mk = lambda ds: DataLoader(ds, hps.batch_size, rank=rank, world=world)       # disjoint per-rank shards of each global batch
        data_loader, source_loader, target_loader = mk(dataset), mk(sourceset), mk(targetset)
        os.makedirs(args.ckpt_dir, exist_ok=True)
        model_path = os.path.join(args.ckpt_dir, args.model_name)
        vq_train = None
        if args.vq_codebook is not None:                  # --vq_train / --rvq_train: the --train_ae loop runs through this codebook
            from zs_amd.vq_train import BETA, DECAY
            vq_train = (args.vq_codebook, args.vq_beta if args.vq_beta is not None else BETA,
                        args.vq_decay if args.vq_decay is not None else DECAY)
            if args.vq_restart is not None:
                vq_train += (args.vq_restart,)
        more = {'rvq_dropout': args.rvq_dropout} if args.rvq_dropout is not None else {}      # --rvq_dropout: with --rvq_train alone
        trainer = Trainer(hps, data_loader, args.g_mode, args.enc_mode, dtype=args.dtype, ema=args.ema, valid=valid, vq_train=vq_train, **more)
        if args.load_model:
            trainer.load_model(os.path.join(args.ckpt_dir, args.load_train_model_name), load_model_list=hps.load_model_list,
                               use_ema=args.use_ema)
        if args.train or args.train_ae:
            trainer.train(model_path, args.flag, mode='pretrain_AE', resume=args.resume)       # stage 1: reconstruction
            trainer.reset_keep()
        if args.train or args.train_p or args.train_tgat:
            trainer.add_duo_loader(source_loader, target_loader)
            trainer.train(model_path, args.flag, mode='patchGAN', target_guided=args.train_tgat, resume=args.resume)
            trainer.reset_keep()
        if args.train_c:                                  # main.py:165-167 (--train keeps the stages above)
            trainer.train(model_path, args.flag, mode='t_classify', resume=args.resume)        # the target speaker classifier
            trainer.reset_keep()
        if args.train and parallel.rank() == 0:
            # reference main.py:163-173 goes on to the autolocker, t_classify and Tacotron stages: outside the path this build covers
            print("[Runner] - --train ran the pretrain_AE and patchGAN stages; the reference's autolocker / t_classify / Tacotron "
                  'stages are not part of this build and were skipped')

    if args.adapt_voice is not None:                      # not in the reference: enrol a new target voice (zs_amd.voice)
        import json
        from zs_amd import voice
        model_path = args.ckpt_pth if args.ckpt_pth is not None else os.path.join(args.ckpt_dir, args.load_test_model_name)
        trainer = get_trainer(args.hps_path, model_path, args.g_mode, args.enc_mode, use_ema=args.use_ema)
        speaker2id = {}
        if os.path.exists(args.speaker2id_path):
            with open(args.speaker2id_path, 'r') as f_json:
                speaker2id = json.load(f_json)
        voice.adapt(trainer, hps.seg_len, args.adapt_dir, args.adapt_voice,
                    args.voice_dir if args.voice_dir is not None else os.path.join(args.ckpt_dir, 'voices'), speaker2id=speaker2id,
                    iters=(args.adapt_iters if args.adapt_iters is not None else voice.ADAPT_ITERS), init=args.adapt_init,
                    lr=args.adapt_lr)

    if args.fit_codebook is not None:                     # not in the reference: a codebook over a folder (zs_amd.codebook, zs_amd.vq)
        from zs_amd.vq import kind_for                    # the model's enc_mode chooses the kind: bits (k-modes) or vectors (k-means)
        model_path = args.ckpt_pth if args.ckpt_pth is not None else os.path.join(args.ckpt_dir, args.load_test_model_name)
        trainer = get_trainer(args.hps_path, model_path, args.g_mode, args.enc_mode, use_ema=args.use_ema)
        iters = args.codebook_iters if args.codebook_iters is not None else CODEBOOK_ITERS
        seed = args.codebook_seed if args.codebook_seed is not None else 0
        if args.rvq is not None:                          # --rvq S: S stages of K codewords, fitted greedily (zs_amd.rvq)
            from zs_amd import rvq
            rvq.fit_dir(trainer, hps.seg_len, args.fit_dir, args.fit_codebook, args.rvq,
                        args.codebook_out if args.codebook_out is not None else
                        rvq.ResidualCodebook.default_path(args.ckpt_dir, args.fit_codebook, args.rvq), iters=iters, seed=seed)
        else:
            kind = kind_for(trainer.enc_mode)
            kind.fit_dir(trainer, hps.seg_len, args.fit_dir, args.fit_codebook,
                         args.codebook_out if args.codebook_out is not None else kind.default_path(args.ckpt_dir, args.fit_codebook),
                         iters=iters, seed=seed)

    if args.test or args.cross_test or args.test_encode or args.test_single or args.test_classify or args.convert_dir is not None or \
            args.synth_dir is not None:
        os.makedirs(args.result_dir, exist_ok=True)
        model_path = args.ckpt_pth if args.ckpt_pth is not None else os.path.join(args.ckpt_dir, args.load_test_model_name)
        trainer = get_trainer(args.hps_path, model_path, args.g_mode, args.enc_mode, args.load_tclf_model_name, use_ema=args.use_ema)
        result_dir = os.path.join(args.result_dir, args.sub_result_dir)
        os.makedirs(result_dir, exist_ok=True)
        cb = None
        if args.codebook is not None:                     # a malformed file or another width: ValueError before anything is enqueued
            from zs_amd.vq import load_codebook       # the file's kind and the model's enc_mode choose the path
            cb = load_codebook(args.codebook, trainer.enc_mode, E=int(trainer.Decoder.c_in))
            if args.rvq_stages is not None:               # (check_rvq has seen that the file is a residual codebook of that many stages)
                cb = cb.with_stages(args.rvq_stages)
            if args.segment is not None or args.segments:     # K > ZS_SEG_MAX_K: refused before anything is enqueued
                from zs_amd import segment as sg
                sg.check_codebook(cb)
                if args.segment is not None:
                    print('[Runner] - Segmenting: lambda = %g per change of codeword, in %s' % (args.segment, sg.unit_name(cb)))
        voices = None
        if args.voice:                                    # --voice NAME=FILE: rows appended to the Decoder's tables (zs_amd.voice)
            from zs_amd.voice import add_voices
            voices = add_voices(trainer, voice_files(args))
        if args.test:
            test_from_list(trainer, hps.seg_len, args.synthesis_list, args.dataset_path, args.speaker2id_path, result_dir, args.enc_only)
        if args.cross_test:                               # main.py:188-189
            cross_test(trainer, hps.seg_len, args.dataset_path, args.speaker2id_path, args.result_dir, args.enc_only, flag='test')
        if args.test_single:                              # main.py:190-191
            test_single(trainer, hps.seg_len, args.speaker2id_path, args.result_dir, args.enc_only, args.s_speaker, args.t_speaker)
        if args.test_encode:
            test_encode(trainer, hps.seg_len, args.test_path, args.dataset_path, result_dir, flag='test', codebook=cb,
                        **({'segment': args.segment} if args.segment is not None else {}))
        if args.test_classify:                            # main.py:196-199
            target_classify(trainer, hps.seg_len, args.synthesis_list, result_dir, flag='test')
        if args.convert_dir is not None:                  # not in the reference: a folder of sound files to the target voices
            convert_dir(trainer, hps.seg_len, args.convert_dir, args.speaker2id_path, os.path.join(result_dir, 'convert'), args.t_speakers,
                        args.enc_only, voices=voices, codebook=cb, codebook_file=args.codebook,
                        **({'overlap': args.overlap} if args.overlap is not None else {}),
                        **({'segment': args.segment} if args.segment is not None else {}))
        if args.synth_dir is not None:                    # not in the reference: a folder of unit files spoken by the target voices
            synth_dir(trainer, hps.seg_len, args.synth_dir, args.speaker2id_path, os.path.join(result_dir, 'synth'), args.t_speakers,
                      args.enc_only, voices=voices, codebook=cb, codebook_file=args.codebook,
                      **({'overlap': args.overlap} if args.overlap is not None else {}), **({'segments': True} if args.segments else {}))


if __name__ == '__main__':
    main()
