// EncodecNative: the managed Encodec model (NeuralCodecs.Torch/Models/Encodec.cs) over libnc_mi355x.so -- the reference's public
// members and properties with the reference's signatures and exceptions; frames are the reference's own EncodedFrame record
// (Modules/Encodec/EncodedFrame.cs).  Checked against the reference's .cs files by tests/test_csharp_shim_cpu.py.
using System;
using System.Collections.Generic;
using System.Linq;
using NeuralCodecs.Core;
using NeuralCodecs.Core.Configuration;
using NeuralCodecs.Torch.Config.Encodec;
using NeuralCodecs.Torch.Modules.Encodec;
using NeuralCodecs.Torch.Native;
using TorchSharp;
using static TorchSharp.torch;

namespace NeuralCodecs.Torch.Models;

public sealed unsafe class EncodecNative : INeuralCodec
{
    private static readonly int[] SeanetRatios = { 8, 5, 4, 2 };                    // SEANetEncoder.cs:55: the config's ratios never reach SEANet (D11)

    private IntPtr _h;
    private readonly EncodecConfig _config;
    private readonly float _overlap;
    private readonly float? _segment;
    private readonly List<float> _targetBandwidths;
    private readonly int _numCodebooks;
    private float? _bandwidth;

    public EncodecNative(EncodecConfig config)                                      // Models/Encodec.cs:46-90
    {
        _config = config ?? throw new ArgumentNullException(nameof(config));
        if (config.Bandwidth is null || !((IList<float>)config.TargetBandwidths).Contains(config.Bandwidth.Value))
        {
            throw new ArgumentException(                                            // Encodec.cs:49-54
                $"Invalid bandwidth {config.Bandwidth}. " +
                $"Select one of [{string.Join(", ", config.TargetBandwidths)}]");
        }
        _targetBandwidths = config.TargetBandwidths.ToList();
        _bandwidth = config.Bandwidth;
        int totalRatio = SeanetRatios.Aggregate((a, b) => a * b);                  // encoder.TotalRatio, SEANetEncoder.cs:140
        _numCodebooks = (int)(1000 * config.TargetBandwidths.Max() /
            (Math.Ceiling(config.SampleRate / (double)totalRatio) * 10));           // Encodec.cs:70-71
        SampleRate = config.SampleRate;
        _segment = config.ChunkLengthSeconds;
        Channels = config.Channels;
        Normalize = config.Normalize;
        _overlap = config.Overlap ?? 0;                                             // Encodec.cs:84
        FrameRate = (int)Math.Ceiling(SampleRate / (float)totalRatio);              // Encodec.cs:86
        BitsPerCodebook = (int)Math.Log2(config.CodebookSize);                      // Encodec.cs:87

        var c = new NcEncodecConfig
        {
            sample_rate = config.SampleRate, channels = config.Channels, dimension = config.HiddenSize, n_filters = 32, n_ratios = 4,
            lstm_layers = 2, compress = 2, kernel_size = 7, last_kernel_size = 7, residual_kernel_size = 3,   // SEANetEncoder.cs:37-56 defaults
            time_group_norm = config.NormType == "time_group_norm" ? 1 : 0, causal = config.UseCausalConv ? 1 : 0,
            normalize = config.Normalize ? 1 : 0, segment_length = SegmentLength ?? 0, segment_stride = SegmentStride ?? 0,
            codebook_size = config.CodebookSize, n_codebooks = _numCodebooks, frame_rate = FrameRate, bandwidth = config.Bandwidth.Value,
        };
        for (int i = 0; i < 4; ++i) c.ratios[i] = SeanetRatios[i];
        NcMi355x.Check(NcMi355x.nc_encodec_create(in c, NcMi355x.DeviceIndex(config.Device), out _h));
    }

    // ---- properties (Models/Encodec.cs:145-201) ---------------------------------------------------------------------------------------
    public int BitsPerCodebook { get; }
    public int Channels { get; }
    public IModelConfig Config => _config;
    public float? CurrentBandwidth => _bandwidth;
    public int FrameRate { get; }
    public bool Normalize { get; }
    public int NumCodebooks => _numCodebooks;
    public int SampleRate { get; }
    public int? SegmentLength => _segment.HasValue ? (int)(_segment.Value * SampleRate) : null;
    public int? SegmentStride => SegmentLength.HasValue ?
        Math.Max(1, (int)((1 - _overlap) * SegmentLength.Value)) : null;
    public IReadOnlyList<float> TargetBandwidths => _targetBandwidths;

    public void LoadWeights(string path)                                            // Models/Encodec.cs:348-385
    {
        if (string.IsNullOrEmpty(path)) throw new ArgumentException("Weights path cannot be empty", nameof(path));
        NcMi355x.Check(NcMi355x.nc_codec_load_weights(_h, path));
    }

    public void SetTargetBandwidth(float bandwidth)                                 // Models/Encodec.cs:409-419
    {
        if (!_targetBandwidths.Contains(bandwidth))
        {
            throw new ArgumentException(
                $"This model doesn't support the bandwidth {bandwidth} kbps. " +
                $"Select one of [{string.Join(", ", _targetBandwidths)} kbps]");
        }
        NcMi355x.Check(NcMi355x.nc_encodec_set_bandwidth(_h, bandwidth));
        _bandwidth = bandwidth;
        _config.Bandwidth = bandwidth;
    }

    // ---- host-array cores ------------------------------------------------------------------------------------------------------------
    /// <summary>x [B,C,T] -> per segment (codes [B,n_q,T'_f], scale [B] or null).  Models/Encodec.cs:259-285, EncodeFrame :457-489.</summary>
    public List<(long[] codes, float[]? scale, int nQ, long frames)> EncodeHost(float[] audio, int B, long T)
    {
        ArgumentNullException.ThrowIfNull(audio);
        int nFrames, nQ;
        long decoded;
        NcMi355x.Check(NcMi355x.nc_encodec_query(_h, T, &nFrames, &nQ, null, 0, &decoded));   // count first
        var lens = new long[nFrames];
        fixed (long* pl = lens) NcMi355x.Check(NcMi355x.nc_encodec_query(_h, T, &nFrames, &nQ, pl, nFrames, &decoded));
        long total = lens.Sum();
        var codes = new long[B * nQ * total];
        var scales = new float[nFrames * B];
        fixed (float* p = audio, ps = scales) fixed (long* pc = codes)
            NcMi355x.Check(NcMi355x.nc_encodec_encode(_h, p, B, T, pc, ps, null));
        var frames = new List<(long[], float[]?, int, long)>(nFrames);
        long off = 0;
        for (int f = 0; f < nFrames; ++f)
        {
            long n = (long)B * nQ * lens[f];
            var c = new long[n];
            Array.Copy(codes, off, c, 0, n);
            float[]? sc = Normalize ? scales.AsSpan(f * B, B).ToArray() : null;
            frames.Add((c, sc, nQ, lens[f]));
            off += n;
        }
        return frames;
    }

    /// <summary>frames -> audio [B,C,decoded]: decode + scale + linear overlap-add (Models/Encodec.cs:213-235,436-455).  The frames
    /// alone fix the output, as in the reference: the clip length of their layout comes from nc_encodec_clip_length.</summary>
    public float[] DecodeHost(List<(long[] codes, float[]? scale, int nQ, long frames)> frames, int B, out long decoded)
    {
        if (frames.Count == 0) throw new ArgumentException("No frames provided to decode");              // Encodec.cs:215-218
        if (SegmentLength == null && frames.Count != 1)
            throw new ArgumentException("Expected single frame when no segmentation is used");              // Encodec.cs:222-225
        long T, dec;
        int nFrames, nQq;
        var lens = frames.ConvertAll(f => f.frames).ToArray();
        fixed (long* pl = lens)
        {
            NcMi355x.Check(NcMi355x.nc_encodec_clip_length(_h, frames.Count, pl, &T));   // NC_EINVAL: no clip is cut into frames of these lengths
            NcMi355x.Check(NcMi355x.nc_encodec_query(_h, T, &nFrames, &nQq, null, 0, &dec));
        }
        int nQ = frames[0].nQ;
        for (int f = 0; f < frames.Count; ++f)
            if (frames[f].nQ != nQ || frames[f].codes.Length != (long)B * nQ * lens[f])
                throw new ArgumentException($"Frame {f}: expected [{B}, {nQ}, {lens[f]}] codes");
        var codes = new long[frames.Sum(f => (long)f.codes.Length)];
        var scales = new float[frames.Count * B];
        long off = 0;
        for (int f = 0; f < frames.Count; ++f)
        {
            Array.Copy(frames[f].codes, 0, codes, off, frames[f].codes.Length);
            off += frames[f].codes.Length;
            if (frames[f].scale is float[] s) Array.Copy(s, 0, scales, f * B, B);
        }
        var pcm = new float[(long)B * Channels * dec];
        fixed (long* pc = codes) fixed (float* ps = scales, pp = pcm)
            NcMi355x.Check(NcMi355x.nc_encodec_decode(_h, pc, Normalize ? ps : null, B, T, nQ, pp));
        decoded = dec;
        return pcm;
    }

    /// <summary>Clips of unequal lengths in one call (whole files): pcmPacked holds clip b, [Channels, lengths[b]], behind clip b-1.
    /// Returns the packed codes -- clip b's part is the codes buffer of EncodeHost(B = 1) on that clip, its frames [nQ, T'_f] end to
    /// end -- with nFrames[b] segments and codeFrames[b] code frames per clip, and the packed scales (nFrames[b] floats per clip).
    /// The segments of all clips run pooled in uniform batches; every clip's result is that of Encode on it alone, bit for bit.</summary>
    public long[] EncodeRagged(float[] pcmPacked, long[] lengths, out int[] nFrames, out long[] codeFrames, out float[] scalesPacked)
    {
        ArgumentNullException.ThrowIfNull(pcmPacked);
        ArgumentNullException.ThrowIfNull(lengths);
        nFrames = new int[lengths.Length];
        codeFrames = new long[lengths.Length];
        int nf, nQ;
        long dec;
        NcMi355x.Check(NcMi355x.nc_encodec_query(_h, 1, &nf, &nQ, null, 0, &dec));                    // n_q of the bandwidth in force
        fixed (long* pl = lengths, pc = codeFrames) fixed (int* pn = nFrames)
            NcMi355x.Check(NcMi355x.nc_encodec_ragged_query(_h, lengths.Length, pl, pn, pc, null));
        var codes = new long[Math.Max(1, nQ * codeFrames.Sum())];
        scalesPacked = new float[Math.Max(1, nFrames.Sum())];
        fixed (float* p = pcmPacked, ps = scalesPacked) fixed (long* pl = lengths, pc = codes)
            NcMi355x.Check(NcMi355x.nc_encodec_encode_ragged(_h, p, lengths.Length, pl, pc, ps, null));
        return codes;
    }

    /// <summary>Decode of clips of unequal lengths in one call: codesPacked / scalesPacked as EncodeRagged returns them, lengths the
    /// clips' sample counts; the packed PCM holds clip b as [Channels, decodedLens[b]].</summary>
    public float[] DecodeRagged(long[] codesPacked, float[]? scalesPacked, long[] lengths, int nQ, out long[] decodedLens)
    {
        ArgumentNullException.ThrowIfNull(codesPacked);
        ArgumentNullException.ThrowIfNull(lengths);
        decodedLens = new long[lengths.Length];
        fixed (long* pl = lengths, pd = decodedLens)
            NcMi355x.Check(NcMi355x.nc_encodec_ragged_query(_h, lengths.Length, pl, null, null, pd));
        var pcm = new float[Math.Max(1, Channels * decodedLens.Sum())];
        fixed (long* pc = codesPacked, pl = lengths) fixed (float* ps = scalesPacked, pp = pcm)
            NcMi355x.Check(NcMi355x.nc_encodec_decode_ragged(_h, pc, Normalize ? ps : null, lengths.Length, pl, nQ, pp));
        return pcm;
    }

    // ---- stream pool: PCM or frames that arrive over time (segmented models; nc_encodec_stream_pool_*) ---------------------------------
    /// <summary>nSlots live streams on this model, one direction, stepped together; what a slot emits, end to end, is Encode / Decode
    /// (with DSP.LinearOverlapAdd) on the whole stream, bit for bit.  The one-stream session is a pool with one slot.  The pool borrows
    /// the model: destroy it first.  nQ (decode): codebooks in the pushed codes, 0 = the bandwidth in force.</summary>
    public IntPtr CreateStreamPool(bool decode, int nSlots, int nQ = 0)
    {
        NcMi355x.Check(NcMi355x.nc_encodec_stream_pool_create(_h, decode ? 1 : 0, nSlots, nQ, out IntPtr p));
        return p;
    }

    public static void DestroyStreamPool(IntPtr pool) => NcMi355x.Check(NcMi355x.nc_encodec_stream_pool_destroy(pool));

    public static void ResetStreamSlot(IntPtr pool, int slot) => NcMi355x.Check(NcMi355x.nc_encodec_stream_pool_reset_slot(pool, slot));

    public static long StreamPending(IntPtr pool, int slot)
    {
        long n;
        NcMi355x.Check(NcMi355x.nc_encodec_stream_pool_pending(pool, slot, &n));
        return n;
    }

    /// <summary>The rows a step would run under the pool's current state, in launch order (clip: the entry's index): per entry its
    /// segments, their offsets in the stream and their code frames.  frameLens: decode pools only.</summary>
    public static NcEncodecRaggedRow[] StreamPlan(IntPtr pool, int[] slots, long[] nIn, int[] flush, long[]? frameLens, out NcEncodecRaggedPlan plan)
    {
        ArgumentNullException.ThrowIfNull(slots);
        ArgumentNullException.ThrowIfNull(nIn);
        ArgumentNullException.ThrowIfNull(flush);
        NcEncodecRaggedPlan p;
        fixed (int* ps = slots, pf = flush) fixed (long* pi = nIn, pl = frameLens)
            NcMi355x.Check(NcMi355x.nc_encodec_stream_pool_plan(pool, slots.Length, ps, pi, pf, pl, &p, null, 0));
        var rows = new NcEncodecRaggedRow[Math.Max(1, (int)p.n_rows)];
        fixed (int* ps = slots, pf = flush) fixed (long* pi = nIn, pl = frameLens) fixed (NcEncodecRaggedRow* pr = rows)
            NcMi355x.Check(NcMi355x.nc_encodec_stream_pool_plan(pool, slots.Length, ps, pi, pf, pl, &p, pr, p.n_rows));
        plan = p;
        return rows;
    }

    /// <summary>One step of an encode pool: entry i pushes nIn[i] samples of slot slots[i] ([Channels, nIn[i]], packed entry after entry)
    /// and ends the stream where flush[i] != 0.  Returns the packed codes of the segments that became complete -- per entry nFrames[i]
    /// segments with codeFrames[i] code frames in all, each laid out as EncodeHost(B = 1) lays it out -- and one scale per segment.</summary>
    public long[] StreamEncodeStep(IntPtr pool, int[] slots, long[] nIn, int[] flush, float[] pcmPacked, out int[] nFrames, out long[] codeFrames,
                                   out float[] scalesPacked)
    {
        ArgumentNullException.ThrowIfNull(slots);
        ArgumentNullException.ThrowIfNull(nIn);
        ArgumentNullException.ThrowIfNull(flush);
        ArgumentNullException.ThrowIfNull(pcmPacked);
        nFrames = new int[slots.Length];
        codeFrames = new long[slots.Length];
        int nf, nQ;
        long dec;
        NcMi355x.Check(NcMi355x.nc_encodec_query(_h, 1, &nf, &nQ, null, 0, &dec));                    // n_q of the bandwidth in force
        fixed (int* ps = slots, pf = flush, pn = nFrames) fixed (long* pi = nIn, pc = codeFrames)
            NcMi355x.Check(NcMi355x.nc_encodec_stream_pool_query(pool, slots.Length, ps, pi, pf, null, pn, pc, null));
        var codes = new long[Math.Max(1, nQ * codeFrames.Sum())];
        scalesPacked = new float[Math.Max(1, nFrames.Sum())];
        fixed (int* ps = slots, pf = flush) fixed (long* pi = nIn, pc = codes) fixed (float* pp = pcmPacked, psc = scalesPacked)
            NcMi355x.Check(NcMi355x.nc_encodec_stream_pool_step(pool, slots.Length, ps, pi, pf, null, pp, null, pc, psc, null, codes.Length, null, null));
        return codes;
    }

    /// <summary>One step of a decode pool: entry i pushes nIn[i] frames of slot slots[i] -- codes [nQ, frameLens[..]] end to end and one
    /// scale per frame, packed entry after entry -- and ends the stream where flush[i] != 0 (its last one or two frames may then be the
    /// clip's short tail).  Returns the packed PCM, [Channels, nSamples[i]] per entry: the samples that became final.</summary>
    public float[] StreamDecodeStep(IntPtr pool, int[] slots, long[] nIn, int[] flush, long[] frameLens, long[] codesPacked, float[]? scalesPacked,
                                    out long[] nSamples)
    {
        ArgumentNullException.ThrowIfNull(slots);
        ArgumentNullException.ThrowIfNull(nIn);
        ArgumentNullException.ThrowIfNull(flush);
        ArgumentNullException.ThrowIfNull(frameLens);
        ArgumentNullException.ThrowIfNull(codesPacked);
        nSamples = new long[slots.Length];
        fixed (int* ps = slots, pf = flush) fixed (long* pi = nIn, pl = frameLens, pn = nSamples)
            NcMi355x.Check(NcMi355x.nc_encodec_stream_pool_query(pool, slots.Length, ps, pi, pf, pl, null, null, pn));
        var pcm = new float[Math.Max(1, Channels * nSamples.Sum())];
        fixed (int* ps = slots, pf = flush) fixed (long* pi = nIn, pl = frameLens, pc = codesPacked) fixed (float* psc = scalesPacked, pp = pcm)
            NcMi355x.Check(NcMi355x.nc_encodec_stream_pool_step(pool, slots.Length, ps, pi, pf, pl, pc, Normalize ? psc : null, pp, null, null, pcm.Length, null, null));
        return pcm;
    }

    // ---- causal streams: PCM or code frames that arrive over time (causal models without segmentation; nc_encodec_causal_pool_*) -----
    /// <summary>nSlots live streams on this causal, unsegmented model (the 24 kHz preset), one direction, stepped together, the SLSTM's
    /// state carried from step to step; what a slot emits, end to end, is Encode / Decode on the whole stream, bit for bit.  The pool
    /// borrows the model: destroy it first.  nQ (decode): codebooks in the pushed codes, 0 = the bandwidth in force.</summary>
    public IntPtr CreateCausalPool(bool decode, int nSlots, int nQ = 0)
    {
        NcMi355x.Check(NcMi355x.nc_encodec_causal_pool_create(_h, decode ? 1 : 0, nSlots, nQ, out IntPtr p));
        return p;
    }

    public static void DestroyCausalPool(IntPtr pool) => NcMi355x.Check(NcMi355x.nc_encodec_causal_pool_destroy(pool));

    public static void ResetCausalSlot(IntPtr pool, int slot) => NcMi355x.Check(NcMi355x.nc_encodec_causal_pool_reset_slot(pool, slot));

    public static long CausalPending(IntPtr pool, int slot)
    {
        long n;
        NcMi355x.Check(NcMi355x.nc_encodec_causal_pool_pending(pool, slot, &n));
        return n;
    }

    /// <summary>The windows a step would run under the pool's current state, in launch order (entry: the entry's index).</summary>
    public static NcEncodecCausalRow[] CausalPlan(IntPtr pool, int[] slots, long[] nIn, int[] flush, out long nBatches)
    {
        ArgumentNullException.ThrowIfNull(slots);
        ArgumentNullException.ThrowIfNull(nIn);
        ArgumentNullException.ThrowIfNull(flush);
        long nr, nb;
        fixed (int* ps = slots, pf = flush) fixed (long* pi = nIn)
            NcMi355x.Check(NcMi355x.nc_encodec_causal_pool_plan(pool, slots.Length, ps, pi, pf, null, 0, &nr, &nb));
        var rows = new NcEncodecCausalRow[Math.Max(1, (int)nr)];
        fixed (int* ps = slots, pf = flush) fixed (long* pi = nIn) fixed (NcEncodecCausalRow* pr = rows)
            NcMi355x.Check(NcMi355x.nc_encodec_causal_pool_plan(pool, slots.Length, ps, pi, pf, pr, nr, &nr, &nb));
        nBatches = nb;
        return rows;
    }

    /// <summary>One step of a causal encode pool: entry i pushes nIn[i] samples of slot slots[i] ([Channels, nIn[i]], packed entry after
    /// entry) and ends the stream where flush[i] != 0.  Returns the packed codes, [nQ, codeFrames[i]] per entry: the frames that became final.</summary>
    public long[] CausalEncodeStep(IntPtr pool, int[] slots, long[] nIn, int[] flush, float[] pcmPacked, out long[] codeFrames)
    {
        ArgumentNullException.ThrowIfNull(slots);
        ArgumentNullException.ThrowIfNull(nIn);
        ArgumentNullException.ThrowIfNull(flush);
        ArgumentNullException.ThrowIfNull(pcmPacked);
        codeFrames = new long[slots.Length];
        int nf, nQ;
        long dec;
        NcMi355x.Check(NcMi355x.nc_encodec_query(_h, 1, &nf, &nQ, null, 0, &dec));                    // n_q of the bandwidth in force
        fixed (int* ps = slots, pf = flush) fixed (long* pi = nIn, pc = codeFrames)
            NcMi355x.Check(NcMi355x.nc_encodec_causal_pool_query(pool, slots.Length, ps, pi, pf, pc));
        var codes = new long[Math.Max(1, nQ * codeFrames.Sum())];
        fixed (int* ps = slots, pf = flush) fixed (long* pi = nIn, pc = codes) fixed (float* pp = pcmPacked)
            NcMi355x.Check(NcMi355x.nc_encodec_causal_pool_step(pool, slots.Length, ps, pi, pf, pp, pc, null, codes.Length, null));
        return codes;
    }

    /// <summary>One step of a causal decode pool: entry i pushes nIn[i] code frames of slot slots[i] ([nQ, nIn[i]], packed entry after
    /// entry) and ends the stream where flush[i] != 0.  Returns the packed PCM, [Channels, nSamples[i]] per entry: the samples that became final.</summary>
    public float[] CausalDecodeStep(IntPtr pool, int[] slots, long[] nIn, int[] flush, long[] codesPacked, out long[] nSamples)
    {
        ArgumentNullException.ThrowIfNull(slots);
        ArgumentNullException.ThrowIfNull(nIn);
        ArgumentNullException.ThrowIfNull(flush);
        ArgumentNullException.ThrowIfNull(codesPacked);
        nSamples = new long[slots.Length];
        fixed (int* ps = slots, pf = flush) fixed (long* pi = nIn, pn = nSamples)
            NcMi355x.Check(NcMi355x.nc_encodec_causal_pool_query(pool, slots.Length, ps, pi, pf, pn));
        var pcm = new float[Math.Max(1, Channels * nSamples.Sum())];
        fixed (int* ps = slots, pf = flush) fixed (long* pi = nIn, pc = codesPacked) fixed (float* pp = pcm)
            NcMi355x.Check(NcMi355x.nc_encodec_causal_pool_step(pool, slots.Length, ps, pi, pf, pc, pp, null, pcm.Length, null));
        return pcm;
    }

    // ---- the reference's members, signature for signature ---------------------------------------------------------------------------
    public Tensor Decode(List<EncodedFrame> encodedFrames)                          // Models/Encodec.cs:213-235
    {
        if (encodedFrames.Count == 0)
        {
            throw new ArgumentException("No frames provided to decode");
        }
        var host = new List<(long[], float[]?, int, long)>(encodedFrames.Count);
        int B = 0;
        foreach (var frame in encodedFrames)
        {
            if (frame.Codes?.IsInvalid != false)
                throw new ArgumentException("Invalid frame codes in Encodec Decode");                      // Encodec.cs:438-442
            B = (int)frame.Codes.shape[0];
            host.Add((NcTensor.Longs(frame.Codes), frame.Scale is null ? null : NcTensor.Floats(frame.Scale),
                      (int)frame.Codes.shape[1], frame.Codes.shape[2]));
        }
        var pcm = DecodeHost(host, B, out long decoded);
        return NcTensor.From(pcm, B, Channels, decoded);
    }

    public List<EncodedFrame> Encode(float[] audioData)                             // Models/Encodec.cs:243-257
    {
        ArgumentNullException.ThrowIfNull(audioData);
        return ToFrames(EncodeHost(audioData, 1, audioData.Length / _config.Channels), 1);   // reshape(1, Channels, -1)
    }

    public List<EncodedFrame> Encode(Tensor x)                                      // Models/Encodec.cs:259-285
    {
        ValidateInputTensor(x);
        long channels = x.size(1);
        if (channels is <= 0 or > 2)
        {
            throw new ArgumentException($"Invalid number of channels: {channels}");
        }
        int B = (int)x.size(0);
        return ToFrames(EncodeHost(NcTensor.Floats(x), B, x.size(2)), B);
    }

    public Tensor forward(Tensor x)                                                 // Models/Encodec.cs:292-296
    {
        var frames = Encode(x);
        return Decode(frames).slice(2, 0, x.size(-1), 1);
    }

    private List<EncodedFrame> ToFrames(List<(long[] codes, float[]? scale, int nQ, long frames)> host, int B)
    {
        return host.ConvertAll(f => new EncodedFrame(NcTensor.From(f.codes, B, f.nQ, f.frames),
                                                     f.scale is null ? null : NcTensor.From(f.scale, B, 1)));   // scale.view(-1, 1), Encodec.cs:479
    }

    private void ValidateInputTensor(Tensor x)                                      // Models/Encodec.cs:491-504
    {
        if (x.dim() != 3)
        {
            throw new ArgumentException(
                $"Expected 3D input tensor [B,C,T], got shape [{string.Join(", ", x.shape)}]");
        }
        if (x.shape[1] != _config.Channels)
        {
            throw new ArgumentException(
                $"Expected {_config.Channels} channels, got {x.shape[1]}");
        }
    }

    public void Dispose()
    {
        if (_h != IntPtr.Zero) { NcMi355x.nc_codec_destroy(_h); _h = IntPtr.Zero; }
        GC.SuppressFinalize(this);
    }

    ~EncodecNative() { if (_h != IntPtr.Zero) NcMi355x.nc_codec_destroy(_h); }
}
