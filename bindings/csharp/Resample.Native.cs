// ResampleNative: band-limited (windowed-sinc, polyphase) resampling over libnc_mi355x.so -- what AudioSignal.ResampleFrac
// (AudioTools/AudioSignal.cs:962-1032) stands for -- for callers without TorchSharp: plain arrays and device pointers in, plain arrays out.
// include/nc_mi355x.h, "band-limited resampling", states every value and why ResampleFrac itself is not mirrored.  A row is one channel of
// one clip: row r is n[r] samples at element off[r] of the buffer and comes out as OutputLength(n[r]) samples at outOff[r].
using System;
using NeuralCodecs.Torch.Native;

namespace NeuralCodecs.Torch.Models;

/// <summary>The filter design (nc_resample_cfg); zero fields stand for julius' defaults (24 zero crossings, rolloff 0.945).</summary>
public sealed class ResampleOptions
{
    public int Zeros;                                                                // 1 .. 64, 0 = 24
    public float Rolloff;                                                            // 0.5 .. 1, 0 = 0.945
}

/// <summary>The geometry of a ratio: U output samples per D input samples, K taps per phase (K4 = K rounded up to four), W samples of
/// edge padding on either side.</summary>
public readonly record struct ResampleGeometry(int U, int D, int W, int K, int K4);

public static unsafe class ResampleNative
{
    private static NcResampleCfg Cfg(ResampleOptions? o) => o is null ? default : new NcResampleCfg { zeros = o.Zeros, rolloff = o.Rolloff };

    /// <summary>ceil(n U / D): the samples a row of n comes out as.</summary>
    public static long OutputLength(long n, int sourceRate, int targetRate)
    {
        long m = NcMi355x.nc_audio_resample_sinc_len(n, sourceRate, targetRate);
        if (m < 0) throw new ArgumentException("rates must be at least 1 and the length in [0, 2^30]");
        return m;
    }

    public static ResampleGeometry Geometry(int sourceRate, int targetRate, ResampleOptions? options = null)
    {
        int u, d, w, k, k4;
        var c = Cfg(options);
        NcMi355x.Check(NcMi355x.nc_audio_resample_sinc_geom(sourceRate, targetRate, c, &u, &d, &w, &k, &k4));
        return new ResampleGeometry(u, d, w, k, k4);
    }

    /// <summary>The filter table h[U][K4], row-major.</summary>
    public static float[] Table(int sourceRate, int targetRate, ResampleOptions? options = null)
    {
        var g = Geometry(sourceRate, targetRate, options);
        var h = new float[(long)g.U * g.K4];
        var c = Cfg(options);
        fixed (float* ph = h)
            NcMi355x.Check(NcMi355x.nc_audio_resample_sinc_table(sourceRate, targetRate, c, ph));
        return h;
    }

    /// <summary>Rows of a HOST array on the device (synchronous): the resampled rows end to end, and where each begins.</summary>
    public static (float[] pcm, long[] off) Resample(int deviceIndex, float[] pcm, long[] off, long[] n, int sourceRate, int targetRate,
                                                     ResampleOptions? options = null)
    {
        CheckSpans(pcm, off, n);
        var (result, outOff) = Allocate(n, sourceRate, targetRate);
        var c = Cfg(options);
        fixed (float* p = pcm, po = result) fixed (long* pf = off, pn = n, poo = outOff)
            NcMi355x.Check(NcMi355x.nc_audio_resample_sinc(deviceIndex, p, n.Length, pf, pn, sourceRate, targetRate, c, po, poo));
        return (result, outOff);
    }

    /// <summary>The same as plain serial host code, no device: the same bits.</summary>
    public static (float[] pcm, long[] off) ResampleHost(float[] pcm, long[] off, long[] n, int sourceRate, int targetRate,
                                                         ResampleOptions? options = null)
    {
        CheckSpans(pcm, off, n);
        var (result, outOff) = Allocate(n, sourceRate, targetRate);
        var c = Cfg(options);
        fixed (float* p = pcm, po = result) fixed (long* pf = off, pn = n, poo = outOff)
            NcMi355x.Check(NcMi355x.nc_audio_resample_sinc_host(p, n.Length, pf, pn, sourceRate, targetRate, c, po, poo));
        return (result, outOff);
    }

    /// <summary>Rows of a DEVICE buffer into outDev at outOff (which must not overlap the input rows), asynchronous on hipStream: the
    /// first link of resample -> level -> EncodeRagged without leaving the device.</summary>
    public static void ResampleDevice(int deviceIndex, IntPtr pcmDev, long[] off, long[] n, int sourceRate, int targetRate, ResampleOptions? options,
                                      IntPtr outDev, long[] outOff, IntPtr hipStream)
    {
        CheckTables(off, n);
        ArgumentNullException.ThrowIfNull(outOff);
        if (outOff.Length != n.Length) throw new ArgumentException("one output offset per row");
        var c = Cfg(options);
        fixed (long* pf = off, pn = n, poo = outOff)
            NcMi355x.Check(NcMi355x.nc_audio_resample_sinc_dev(deviceIndex, (float*)pcmDev, n.Length, pf, pn, sourceRate, targetRate, c, (float*)outDev, poo,
                                                               (void*)hipStream));
    }

    private static (float[] pcm, long[] off) Allocate(long[] n, int sourceRate, int targetRate)
    {
        var outOff = new long[n.Length];
        long total = 0;
        for (int r = 0; r < n.Length; r++)
        {
            outOff[r] = total;
            total += OutputLength(n[r], sourceRate, targetRate);
        }
        return (new float[Math.Max(total, 1)], outOff);
    }

    private static void CheckTables(long[] off, long[] n)
    {
        ArgumentNullException.ThrowIfNull(off);
        ArgumentNullException.ThrowIfNull(n);
        if (off.Length != n.Length) throw new ArgumentException("one offset per row");
    }

    private static void CheckSpans(float[] pcm, long[] off, long[] n)
    {
        ArgumentNullException.ThrowIfNull(pcm);
        CheckTables(off, n);
        for (int r = 0; r < off.Length; r++)
            if (n[r] < 0 || off[r] < 0 || off[r] + n[r] > pcm.LongLength)
                throw new ArgumentException($"row {r} reaches outside its buffer");
    }
}
