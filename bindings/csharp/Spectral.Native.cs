// SpectralNative: inverse STFT, spectral masks and MFCC over libnc_mi355x.so -- DSP.InverseSTFT, DSP.MaskFrequencies, DSP.MaskTimesteps and
// DSP.MFCC (AudioTools/AudioTensorDSP.cs:124-151, 307-394, 408-441) -- for callers without TorchSharp: plain arrays and device pointers in,
// plain arrays out.  include/nc_mi355x.h, "inverse STFT, spectral masks, MFCC", states every value and the two deviations (unmasked bins
// keep their bits; the DCT matrix has n_mfcc rows).  A spectrogram buffer holds (re, im) float pairs: row b is complex [W/2+1][frames[b]]
// at COMPLEX element specOff[b], as the forward transform writes it.
using System;
using NeuralCodecs.Torch.Native;

namespace NeuralCodecs.Torch.Models;

public static unsafe class SpectralNative
{
    public const int WindowHann = 0, WindowOnes = 1;

    /// <summary>H (frames - 1): the samples torch.istft returns with center = true and no length.</summary>
    public static long OutputLength(long frames, int window, int hop)
    {
        long m = NcMi355x.nc_audio_istft_len(frames, window, hop);
        if (m < 0) throw new ArgumentException("at least one frame, a window of at least 2 and a hop of at least 1");
        return m;
    }

    /// <summary>The synthesis basis T[W][W + 2], row-major.</summary>
    public static float[] Basis(int windowLength, int windowType = WindowHann)
    {
        var t = new float[(long)windowLength * (windowLength + 2)];
        fixed (float* pt = t)
            NcMi355x.Check(NcMi355x.nc_audio_idft_basis(windowLength, windowType, pt));
        return t;
    }

    /// <summary>The orthonormal DCT-II [nMfcc][nMels], row-major.</summary>
    public static float[] DctMatrix(int nMfcc, int nMels)
    {
        if (nMfcc < 1 || nMels < 1) throw new ArgumentException("nMfcc and nMels must be positive");
        var d = new float[(long)nMfcc * nMels];
        fixed (float* pd = d)
            NcMi355x.Check(NcMi355x.nc_audio_dct_matrix(nMfcc, nMels, pd));
        return d;
    }

    /// <summary>The cap in bytes on the frame scratch of one group of rows: set &gt; 0 sets it, -1 restores the default, 0 keeps it.</summary>
    public static long Workspace(int deviceIndex, long set = 0)
    {
        long cap;
        NcMi355x.Check(NcMi355x.nc_audio_istft_workspace(deviceIndex, set, &cap));
        return cap;
    }

    /// <summary>Rows of a HOST spectrogram buffer on the device (synchronous): the PCM rows end to end, and where each begins.
    /// length[b] = 0 (or length = null) stands for OutputLength(frames[b]).</summary>
    public static (float[] pcm, long[] off) InverseSTFT(int deviceIndex, float[] spec, long[] specOff, long[] frames, int windowLength, int hop,
                                                        int windowType = WindowHann, long[]? length = null)
    {
        CheckSpans(spec, specOff, frames, windowLength / 2 + 1);
        var (result, outOff) = Allocate(frames, windowLength, hop, length);
        fixed (float* p = spec, po = result) fixed (long* pf = specOff, pn = frames, poo = outOff, pl = length)
            NcMi355x.Check(NcMi355x.nc_audio_istft(deviceIndex, p, frames.Length, pf, pn, windowLength, hop, windowType, po, poo, pl));
        return (result, outOff);
    }

    /// <summary>The same as plain serial host code, no device: the same bits.</summary>
    public static (float[] pcm, long[] off) InverseSTFTHost(float[] spec, long[] specOff, long[] frames, int windowLength, int hop,
                                                            int windowType = WindowHann, long[]? length = null)
    {
        CheckSpans(spec, specOff, frames, windowLength / 2 + 1);
        var (result, outOff) = Allocate(frames, windowLength, hop, length);
        fixed (float* p = spec, po = result) fixed (long* pf = specOff, pn = frames, poo = outOff, pl = length)
            NcMi355x.Check(NcMi355x.nc_audio_istft_host(p, frames.Length, pf, pn, windowLength, hop, windowType, po, poo, pl));
        return (result, outOff);
    }

    /// <summary>Rows of a DEVICE spectrogram buffer into outDev at outOff, asynchronous on hipStream.</summary>
    public static void InverseSTFTDevice(int deviceIndex, IntPtr specDev, long[] specOff, long[] frames, int windowLength, int hop, int windowType,
                                         IntPtr outDev, long[] outOff, long[]? length, IntPtr hipStream)
    {
        CheckTables(specOff, frames);
        ArgumentNullException.ThrowIfNull(outOff);
        if (outOff.Length != frames.Length || (length is not null && length.Length != frames.Length)) throw new ArgumentException("one entry per row");
        fixed (long* pf = specOff, pn = frames, poo = outOff, pl = length)
            NcMi355x.Check(NcMi355x.nc_audio_istft_dev(deviceIndex, (float*)specDev, frames.Length, pf, pn, windowLength, hop, windowType, (float*)outDev, poo, pl,
                                                       (void*)hipStream));
    }

    /// <summary>The bins [lo, hi) that DSP.MaskFrequencies masks: fminHz &lt;= k (sampleRate / 2) / (nbins - 1) &lt; fmaxHz.</summary>
    public static (int lo, int hi) MaskFrequencyBins(int sampleRate, int nbins, float fminHz, float fmaxHz)
    {
        int lo, hi;
        NcMi355x.Check(NcMi355x.nc_audio_mask_freq_bins(sampleRate, nbins, fminHz, fmaxHz, &lo, &hi));
        return (lo, hi);
    }

    /// <summary>The frames [lo, hi) that DSP.MaskTimesteps masks: tminS &lt;= t duration / (frames - 1) &lt; tmaxS.</summary>
    public static (long lo, long hi) MaskTimeFrames(float signalDuration, long frames, float tminS, float tmaxS)
    {
        long lo, hi;
        NcMi355x.Check(NcMi355x.nc_audio_mask_time_frames(signalDuration, frames, tminS, tmaxS, &lo, &hi));
        return (lo, hi);
    }

    /// <summary>Per row the rectangle [kLo, kHi) x [tLo, tHi) of a HOST spectrogram buffer set to val exp(i val), in place; every other bin
    /// keeps its bits.</summary>
    public static void FillHost(float[] spec, long[] specOff, long[] frames, int nbins, int[] kLo, int[] kHi, long[] tLo, long[] tHi, float val = 0.0f)
    {
        CheckSpans(spec, specOff, frames, nbins);
        CheckRects(frames.Length, kLo, kHi, tLo, tHi);
        fixed (float* p = spec) fixed (long* pf = specOff, pn = frames, ptl = tLo, pth = tHi) fixed (int* pkl = kLo, pkh = kHi)
            NcMi355x.Check(NcMi355x.nc_audio_spec_fill_host(p, frames.Length, pf, pn, nbins, pkl, pkh, ptl, pth, val));
    }

    /// <summary>The same on a DEVICE spectrogram buffer, one launch for all rows, asynchronous on hipStream.</summary>
    public static void FillDevice(int deviceIndex, IntPtr specDev, long[] specOff, long[] frames, int nbins, int[] kLo, int[] kHi, long[] tLo, long[] tHi,
                                  float val, IntPtr hipStream)
    {
        CheckTables(specOff, frames);
        CheckRects(frames.Length, kLo, kHi, tLo, tHi);
        fixed (long* pf = specOff, pn = frames, ptl = tLo, pth = tHi) fixed (int* pkl = kLo, pkh = kHi)
            NcMi355x.Check(NcMi355x.nc_audio_spec_fill_dev(deviceIndex, (float*)specDev, frames.Length, pf, pn, nbins, pkl, pkh, ptl, pth, val, (void*)hipStream));
    }

    /// <summary>MFCC of the rows of a HOST PCM buffer as plain serial host code: row b is [nMfcc][1 + n[b] / hop] at the returned offset.</summary>
    public static (float[] mfcc, long[] off) MfccHost(float[] pcm, long[] off, long[] n, int sampleRate, int windowLength, int hop, int nMfcc = 40,
                                                      int nMels = 80, float melFmin = 0.0f, float melFmax = 0.0f, float logOffset = 1e-6f)
    {
        ArgumentNullException.ThrowIfNull(pcm);
        CheckTables(off, n);
        if (hop < 1) throw new ArgumentException("the hop must be at least 1");
        var outOff = new long[n.Length];
        long total = 0;
        for (int r = 0; r < n.Length; r++)
        {
            if (n[r] < 0 || off[r] < 0 || off[r] + n[r] > pcm.LongLength) throw new ArgumentException($"row {r} reaches outside its buffer");
            outOff[r] = total;
            total += nMfcc * (1 + n[r] / hop);
        }
        var result = new float[Math.Max(total, 1)];
        fixed (float* p = pcm, po = result) fixed (long* pf = off, pn = n, poo = outOff)
            NcMi355x.Check(NcMi355x.nc_audio_mfcc_host(p, n.Length, pf, pn, sampleRate, windowLength, hop, nMels, melFmin, melFmax, nMfcc, logOffset, po, poo));
        return (result, outOff);
    }

    /// <summary>MFCC of the rows of a DEVICE PCM buffer into outDev at outOff, asynchronous on hipStream.</summary>
    public static void MfccDevice(int deviceIndex, IntPtr pcmDev, long[] off, long[] n, int sampleRate, int windowLength, int hop, int nMfcc, int nMels,
                                  float melFmin, float melFmax, float logOffset, IntPtr outDev, long[] outOff, IntPtr hipStream)
    {
        CheckTables(off, n);
        ArgumentNullException.ThrowIfNull(outOff);
        if (outOff.Length != n.Length) throw new ArgumentException("one output offset per row");
        fixed (long* pf = off, pn = n, poo = outOff)
            NcMi355x.Check(NcMi355x.nc_audio_mfcc_dev(deviceIndex, (float*)pcmDev, n.Length, pf, pn, sampleRate, windowLength, hop, nMels, melFmin, melFmax, nMfcc,
                                                      logOffset, (float*)outDev, poo, (void*)hipStream));
    }

    private static (float[] pcm, long[] off) Allocate(long[] frames, int windowLength, int hop, long[]? length)
    {
        if (length is not null && length.Length != frames.Length) throw new ArgumentException("one length per row");
        var outOff = new long[frames.Length];
        long total = 0;
        for (int r = 0; r < frames.Length; r++)
        {
            outOff[r] = total;
            total += length is not null && length[r] != 0 ? length[r] : OutputLength(frames[r], windowLength, hop);
        }
        return (new float[Math.Max(total, 1)], outOff);
    }

    private static void CheckTables(long[] off, long[] n)
    {
        ArgumentNullException.ThrowIfNull(off);
        ArgumentNullException.ThrowIfNull(n);
        if (off.Length != n.Length) throw new ArgumentException("one offset per row");
    }

    private static void CheckRects(int rows, int[] kLo, int[] kHi, long[] tLo, long[] tHi)
    {
        ArgumentNullException.ThrowIfNull(kLo);
        ArgumentNullException.ThrowIfNull(kHi);
        ArgumentNullException.ThrowIfNull(tLo);
        ArgumentNullException.ThrowIfNull(tHi);
        if (kLo.Length != rows || kHi.Length != rows || tLo.Length != rows || tHi.Length != rows) throw new ArgumentException("one rectangle per row");
    }

    private static void CheckSpans(float[] spec, long[] specOff, long[] frames, int nbins)
    {
        ArgumentNullException.ThrowIfNull(spec);
        CheckTables(specOff, frames);
        for (int r = 0; r < specOff.Length; r++)
            if (frames[r] < 1 || specOff[r] < 0 || 2 * (specOff[r] + nbins * frames[r]) > spec.LongLength)
                throw new ArgumentException($"row {r} reaches outside its buffer");
    }
}
