// LoudnessNative: BS.1770 loudness over libnc_mi355x.so -- what the reference computes with LoudnessMeter.IntegratedLoudness /
// NormalizeAudio (AudioTools/LoudnessMeter.cs:127-207) and AudioSignal.Loudness / Normalize (AudioTools/AudioSignal.cs:847-940) -- for
// callers without TorchSharp: plain arrays and device pointers in, plain arrays and structs out.  include/nc_mi355x.h, "loudness", states
// every value.  A clip has C planar channels of one length: channel c of clip b starts at off[b * C + c] of the buffer.
using System;
using NeuralCodecs.Torch.Native;

namespace NeuralCodecs.Torch.Models;

/// <summary>The coefficient source and the target level (nc_loudness_cfg).</summary>
public sealed class LoudnessOptions
{
    public bool DesignedFilter;                                                      // false: the literals of LoudnessMeter.cs:41-52 at any rate
    public float TargetDb = -24.0f;                                                  // LoudnessMeter.NormalizeAudio's default
}

/// <summary>The measurement of one clip.  Gain leads from Lufs to the target; a clip with BadSamples != 0 has NaN in both.</summary>
public readonly record struct LoudnessRow(float Lufs, float Gain, int Blocks, int PassAbsolute, int PassRelative, int BadSamples);

public static unsafe class LoudnessNative
{
    public const float GAIN_FACTOR = 0.11512925464970229f;                           // LoudnessMeter.cs:14

    private static NcLoudnessCfg Cfg(LoudnessOptions o)
    {
        ArgumentNullException.ThrowIfNull(o);
        return new NcLoudnessCfg { filter = o.DesignedFilter ? NcMi355x.NC_KWEIGHT_DESIGNED : NcMi355x.NC_KWEIGHT_REFERENCE, target_db = o.TargetDb };
    }

    private static LoudnessRow[] Rows(NcLoudnessRow[] raw)
    {
        var rows = new LoudnessRow[raw.Length];
        for (int b = 0; b < raw.Length; b++)
            rows[b] = new LoudnessRow(raw[b].lufs, raw[b].gain, raw[b].n_blocks, raw[b].n_pass_abs, raw[b].n_pass_rel, raw[b].n_bad);
        return rows;
    }

    /// <summary>The K-weighting coefficients as (b, a), [2, 3] row-major each: stage 0 the high shelf, stage 1 the high pass.</summary>
    public static (double[] b, double[] a) KWeightCoefficients(int sampleRate, bool designed = false)
    {
        var b = new double[6];
        var a = new double[6];
        fixed (double* pb = b, pa = a)
            NcMi355x.Check(NcMi355x.nc_audio_kweight_coeffs(sampleRate, designed ? NcMi355x.NC_KWEIGHT_DESIGNED : NcMi355x.NC_KWEIGHT_REFERENCE, pb, pa));
        return (b, a);
    }

    /// <summary>IntegratedLoudness of clips in a HOST array on the device (synchronous).</summary>
    public static LoudnessRow[] Measure(int deviceIndex, float[] pcm, int channels, long[] off, long[] n, int sampleRate, LoudnessOptions options)
    {
        CheckSpans(pcm, channels, off, n);
        var c = Cfg(options);
        var raw = new NcLoudnessRow[n.Length];
        fixed (float* p = pcm) fixed (long* po = off, pn = n) fixed (NcLoudnessRow* pr = raw)
            NcMi355x.Check(NcMi355x.nc_loudness(deviceIndex, p, n.Length, channels, po, pn, sampleRate, c, pr));
        return Rows(raw);
    }

    /// <summary>The same as plain serial host code, no device: the same bits.</summary>
    public static LoudnessRow[] MeasureHost(float[] pcm, int channels, long[] off, long[] n, int sampleRate, LoudnessOptions options)
    {
        CheckSpans(pcm, channels, off, n);
        var c = Cfg(options);
        var raw = new NcLoudnessRow[n.Length];
        fixed (float* p = pcm) fixed (long* po = off, pn = n) fixed (NcLoudnessRow* pr = raw)
            NcMi355x.Check(NcMi355x.nc_loudness_host(p, n.Length, channels, po, pn, sampleRate, c, pr));
        return Rows(raw);
    }

    /// <summary>NormalizeAudio in place on a HOST array (synchronous); the rows hold the measured levels for a later Restore.</summary>
    public static LoudnessRow[] Normalize(int deviceIndex, float[] pcm, int channels, long[] off, long[] n, int sampleRate, LoudnessOptions options)
    {
        CheckSpans(pcm, channels, off, n);
        var c = Cfg(options);
        var raw = new NcLoudnessRow[n.Length];
        fixed (float* p = pcm) fixed (long* po = off, pn = n) fixed (NcLoudnessRow* pr = raw)
            NcMi355x.Check(NcMi355x.nc_loudness_normalize(deviceIndex, p, n.Length, channels, po, pn, sampleRate, c, p, po, pr));
        return Rows(raw);
    }

    /// <summary>Clip b times exp(db[b] * GAIN_FACTOR), in place on a HOST array (synchronous).</summary>
    public static void ApplyGainDb(int deviceIndex, float[] pcm, int channels, long[] off, long[] n, float[] db)
    {
        CheckSpans(pcm, channels, off, n);
        ArgumentNullException.ThrowIfNull(db);
        if (db.Length != n.Length) throw new ArgumentException("one gain per clip");
        fixed (float* p = pcm, pd = db) fixed (long* po = off, pn = n)
            NcMi355x.Check(NcMi355x.nc_audio_apply_gain_db(deviceIndex, p, n.Length, channels, po, pn, pd, p, po));
    }

    /// <summary>The gains in dB that lead clips levelled by Normalize back to their measured levels (after a decode).</summary>
    public static float[] RestoreDb(LoudnessRow[] rows, float targetDb)
    {
        ArgumentNullException.ThrowIfNull(rows);
        var db = new float[rows.Length];
        for (int b = 0; b < rows.Length; b++) db[b] = rows[b].Lufs - targetDb;
        return db;
    }

    /// <summary>Clips in a DEVICE buffer, rows out into a DEVICE array of nc_loudness_row (asynchronous on hipStream).</summary>
    public static void MeasureDevice(int deviceIndex, IntPtr pcmDev, int channels, long[] off, long[] n, int sampleRate, LoudnessOptions options,
                                     IntPtr rowsDev, IntPtr hipStream)
    {
        CheckTables(channels, off, n);
        var c = Cfg(options);
        fixed (long* po = off, pn = n)
            NcMi355x.Check(NcMi355x.nc_loudness_dev(deviceIndex, (float*)pcmDev, n.Length, channels, po, pn, sampleRate, c, (NcLoudnessRow*)rowsDev,
                                                    (void*)hipStream));
    }

    /// <summary>Measure and level clips of a DEVICE buffer into outDev at outOff (may equal pcmDev / off: the packed buffer of a ragged
    /// encode, in place), asynchronous on hipStream.</summary>
    public static void NormalizeDevice(int deviceIndex, IntPtr pcmDev, int channels, long[] off, long[] n, int sampleRate, LoudnessOptions options,
                                       IntPtr outDev, long[] outOff, IntPtr rowsDev, IntPtr hipStream)
    {
        CheckTables(channels, off, n);
        ArgumentNullException.ThrowIfNull(outOff);
        if (outOff.Length != off.Length) throw new ArgumentException("one output offset per channel of every clip");
        var c = Cfg(options);
        fixed (long* po = off, pn = n, poo = outOff)
            NcMi355x.Check(NcMi355x.nc_loudness_normalize_dev(deviceIndex, (float*)pcmDev, n.Length, channels, po, pn, sampleRate, c, (float*)outDev, poo,
                                                              (NcLoudnessRow*)rowsDev, (void*)hipStream));
    }

    /// <summary>Clip b of a DEVICE buffer times exp(db[b] * GAIN_FACTOR) into outDev at outOff, asynchronous on hipStream.</summary>
    public static void ApplyGainDbDevice(int deviceIndex, IntPtr pcmDev, int channels, long[] off, long[] n, float[] db, IntPtr outDev, long[] outOff,
                                         IntPtr hipStream)
    {
        CheckTables(channels, off, n);
        ArgumentNullException.ThrowIfNull(db);
        ArgumentNullException.ThrowIfNull(outOff);
        if (db.Length != n.Length || outOff.Length != off.Length) throw new ArgumentException("one gain per clip, one output offset per channel");
        fixed (float* pd = db) fixed (long* po = off, pn = n, poo = outOff)
            NcMi355x.Check(NcMi355x.nc_audio_apply_gain_db_dev(deviceIndex, (float*)pcmDev, n.Length, channels, po, pn, pd, (float*)outDev, poo,
                                                               (void*)hipStream));
    }

    private static void CheckTables(int channels, long[] off, long[] n)
    {
        ArgumentNullException.ThrowIfNull(off);
        ArgumentNullException.ThrowIfNull(n);
        if (channels < 1 || channels > NcMi355x.NC_LOUDNESS_MAX_CHANNELS) throw new ArgumentOutOfRangeException(nameof(channels));
        if (off.Length != (long)n.Length * channels) throw new ArgumentException("one offset per channel of every clip");
    }

    private static void CheckSpans(float[] pcm, int channels, long[] off, long[] n)
    {
        ArgumentNullException.ThrowIfNull(pcm);
        CheckTables(channels, off, n);
        for (int r = 0; r < off.Length; r++)
            if (n[r / channels] < 0 || off[r] < 0 || off[r] + n[r / channels] > pcm.LongLength)
                throw new ArgumentException($"row {r} reaches outside its buffer");
    }
}
