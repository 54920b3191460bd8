// QualityNative: round-trip quality over libnc_mi355x.so -- what the reference computes with DSP.STFT / DSP.MelSpectrogram
// (AudioTools/AudioTensorDSP.cs:595-894) and L1Loss / SISDRLoss / MelSpectrogramLoss (Modules/DAC/) -- for callers without TorchSharp:
// plain arrays and device pointers in, plain arrays and structs out.  include/nc_mi355x.h, "round-trip quality", states every value.
using System;
using NeuralCodecs.Torch.Native;

namespace NeuralCodecs.Torch.Models;

/// <summary>One scale set of the mel distance (nc_quality_cfg).</summary>
public sealed class QualityScales
{
    public int[] Windows = { 32, 64, 128, 256, 512, 1024, 2048 };                   // the DAC paper's evaluation set
    public int[] Mels = { 5, 10, 20, 40, 80, 160, 320 };
    public int[]? Hops;                                                              // null: W / 4
    public float[]? MelFmin;                                                         // null: 0
    public float?[]? MelFmax;                                                        // null entries: sampleRate / 2
    public float ClampEps = 1e-5f, LogWeight = 1.0f, MagWeight = 1.0f;              // MelSpectrogramLoss.cs:33-35

    /// <summary>The constructor defaults of MelSpectrogramLoss (MelSpectrogramLoss.cs:44-45).</summary>
    public static QualityScales ReferenceDefault() => new QualityScales { Windows = new[] { 2048, 512 }, Mels = new[] { 150, 80 } };
}

/// <summary>The metrics of one row: one channel of one clip (SISDRLoss.PrepareInputs).</summary>
public readonly record struct QualityRow(float L1, float SiSdrDb, float MelDistance, float[] MelLog, float[] MelMag, int BadSamples);

public static unsafe class QualityNative
{
    private static NcQualityCfg Cfg(QualityScales s)
    {
        ArgumentNullException.ThrowIfNull(s);
        if (s.Windows.Length < 1 || s.Windows.Length > NcMi355x.NC_QUALITY_MAX_SCALES || s.Mels.Length != s.Windows.Length)
            throw new ArgumentException("All parameter arrays must have same length");   // MelSpectrogramLoss.cs:51-56
        var c = new NcQualityCfg { n_scales = s.Windows.Length, clamp_eps = s.ClampEps, log_weight = s.LogWeight, mag_weight = s.MagWeight };
        for (int i = 0; i < s.Windows.Length; i++)
        {
            c.W[i] = s.Windows[i];
            c.n_mels[i] = s.Mels[i];
            c.H[i] = s.Hops != null ? s.Hops[i] : 0;
            c.fmin[i] = s.MelFmin != null ? s.MelFmin[i] : 0f;
            c.fmax[i] = s.MelFmax != null && s.MelFmax[i].HasValue ? s.MelFmax[i]!.Value : 0f;
        }
        return c;
    }

    private static QualityRow[] Rows(NcQualityRow[] raw, int scales)
    {
        var rows = new QualityRow[raw.Length];
        for (int b = 0; b < raw.Length; b++)
        {
            var lg = new float[scales];
            var mg = new float[scales];
            for (int i = 0; i < scales; i++)
            {
                lg[i] = raw[b].mel_log[i];
                mg[i] = raw[b].mel_mag[i];
            }
            rows[b] = new QualityRow(raw[b].l1, raw[b].si_sdr_db, raw[b].mel_distance, lg, mg, raw[b].n_bad);
        }
        return rows;
    }

    /// <summary>Frames of DSP.STFT (center = true) on n samples; -1 where n &lt;= windowLength / 2.</summary>
    public static long StftFrames(long n, int windowLength, int hopLength) => NcMi355x.nc_audio_stft_frames(n, windowLength, hopLength);

    /// <summary>DSP.MelFilterbank in binary64, rounded once: [nMels, nFft / 2 + 1] row-major.</summary>
    public static float[] MelFilterbank(int sampleRate, int nMels, int nFft, float fMin = 0f, float? fMax = null)   // AudioTensorDSP.cs:844-894
    {
        if (nMels <= 0) throw new ArgumentOutOfRangeException(nameof(nMels), "Number of mel bands must be positive");
        var fb = new float[(long)nMels * (nFft / 2 + 1)];
        fixed (float* p = fb)
            NcMi355x.Check(NcMi355x.nc_audio_mel_filterbank(sampleRate, nMels, nFft, fMin, fMax ?? 0f, p, null, null));
        return fb;
    }

    /// <summary>Metrics of rows in HOST arrays on the device (synchronous): row b is refOff[b] / estOff[b] .. + n[b] of the two buffers.</summary>
    public static QualityRow[] Metrics(int deviceIndex, float[] reference, long[] refOff, float[] estimate, long[] estOff, long[] n, int sampleRate,
                                       QualityScales scales)
    {
        ArgumentNullException.ThrowIfNull(reference);
        ArgumentNullException.ThrowIfNull(estimate);
        ArgumentNullException.ThrowIfNull(n);
        CheckSpans(reference.LongLength, refOff, estimate.LongLength, estOff, n);
        var c = Cfg(scales);
        var raw = new NcQualityRow[n.Length];
        fixed (float* pr = reference, pe = estimate) fixed (long* por = refOff, poe = estOff, pn = n) fixed (NcQualityRow* po = raw)
            NcMi355x.Check(NcMi355x.nc_quality_metrics(deviceIndex, pr, por, pe, poe, pn, n.Length, sampleRate, c, po));
        return Rows(raw, c.n_scales);
    }

    /// <summary>The same as plain serial host code, no device: the same bits.</summary>
    public static QualityRow[] MetricsHost(float[] reference, long[] refOff, float[] estimate, long[] estOff, long[] n, int sampleRate, QualityScales scales)
    {
        ArgumentNullException.ThrowIfNull(reference);
        ArgumentNullException.ThrowIfNull(estimate);
        ArgumentNullException.ThrowIfNull(n);
        CheckSpans(reference.LongLength, refOff, estimate.LongLength, estOff, n);
        var c = Cfg(scales);
        var raw = new NcQualityRow[n.Length];
        fixed (float* pr = reference, pe = estimate) fixed (long* por = refOff, poe = estOff, pn = n) fixed (NcQualityRow* po = raw)
            NcMi355x.Check(NcMi355x.nc_quality_metrics_host(pr, por, pe, poe, pn, n.Length, sampleRate, c, po));
        return Rows(raw, c.n_scales);
    }

    /// <summary>Rows in DEVICE buffers, rows out into a DEVICE array of nc_quality_row (asynchronous on hipStream): the packed input of a
    /// ragged encode against the packed output of the ragged decode, in place.</summary>
    public static void MetricsDevice(int deviceIndex, IntPtr referenceDev, long[] refOff, IntPtr estimateDev, long[] estOff, long[] n, int sampleRate,
                                     QualityScales scales, IntPtr rowsDev, IntPtr hipStream)
    {
        ArgumentNullException.ThrowIfNull(refOff);
        ArgumentNullException.ThrowIfNull(estOff);
        ArgumentNullException.ThrowIfNull(n);
        if (refOff.Length != n.Length || estOff.Length != n.Length) throw new ArgumentException("one offset per row in both buffers");
        var c = Cfg(scales);
        fixed (long* por = refOff, poe = estOff, pn = n)
            NcMi355x.Check(NcMi355x.nc_quality_metrics_dev(deviceIndex, (float*)referenceDev, por, (float*)estimateDev, poe, pn, n.Length, sampleRate, c,
                                                           (NcQualityRow*)rowsDev, (void*)hipStream));
    }

    private static void CheckSpans(long refLen, long[] refOff, long estLen, long[] estOff, long[] n)
    {
        ArgumentNullException.ThrowIfNull(refOff);
        ArgumentNullException.ThrowIfNull(estOff);
        if (refOff.Length != n.Length || estOff.Length != n.Length) throw new ArgumentException("one offset per row in both buffers");
        for (int b = 0; b < n.Length; b++)
            if (n[b] < 0 || refOff[b] < 0 || estOff[b] < 0 || refOff[b] + n[b] > refLen || estOff[b] + n[b] > estLen)
                throw new ArgumentException($"row {b} reaches outside its buffer");
    }
}
