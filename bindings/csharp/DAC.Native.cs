// DACNative: the managed DAC model (NeuralCodecs.Torch/Models/DAC.cs) over libnc_mi355x.so.
// Every public member of the reference class is here with the reference's signature, exceptions and INeuralCodec contract; TorchSharp
// tensors exist at the API surface only (marshalled through host arrays) -- no TorchSharp operator runs between a member's entry
// and its return.  Checked mechanically against the reference's own .cs files by tests/test_csharp_shim_cpu.py (dotnet is not
// in the build image): config properties by name and type, member signatures, exception constructors, NcMi355x call arity.
using System;
using System.Collections.Generic;
using NeuralCodecs.Core;
using NeuralCodecs.Core.Configuration;
using NeuralCodecs.Torch.Config.DAC;
using NeuralCodecs.Torch.Native;
using TorchSharp;
using static TorchSharp.torch;

namespace NeuralCodecs.Torch.Models;

public sealed unsafe class DACNative : INeuralCodec
{
    private IntPtr _h;
    private readonly DACConfig _config;
    private readonly int _latentDim;
    private readonly int _hopLength;

    public IModelConfig Config => _config;                                          // Models/DAC.cs:38

    public DACNative(DACConfig config)                                              // Models/DAC.cs:51-93
    {
        _config = config ?? throw new ArgumentNullException(nameof(config));
        config.EncoderRates ??= [2, 4, 8, 8];                                       // DAC.cs:57
        config.DecoderRates ??= [8, 8, 4, 2];                                       // DAC.cs:59
        _latentDim = config.LatentDim ?? config.EncoderDim * (1 << config.EncoderRates.Length);   // DAC.cs:63
        _hopLength = 1;
        foreach (int r in config.EncoderRates) _hopLength *= r;                     // DAC.cs:66
        var c = new NcDacConfig
        {
            sample_rate = config.SampleRate, encoder_dim = config.EncoderDim, n_encoder_rates = config.EncoderRates.Length,
            decoder_dim = config.DecoderDim, n_decoder_rates = config.DecoderRates.Length, latent_dim = config.LatentDim ?? 0,
            n_codebooks = config.NumCodebooks, codebook_size = config.CodebookSize, codebook_dim = config.CodebookDim,
        };
        for (int i = 0; i < config.EncoderRates.Length; ++i) c.encoder_rates[i] = config.EncoderRates[i];
        for (int i = 0; i < config.DecoderRates.Length; ++i) c.decoder_rates[i] = config.DecoderRates[i];
        NcMi355x.Check(NcMi355x.nc_dac_create(in c, NcMi355x.DeviceIndex(config.Device), out _h));
    }

    public void LoadWeights(string path)                                            // Models/DAC.cs:345-389 (NCWB blob: tools/convert_checkpoint.py)
    {
        if (string.IsNullOrEmpty(path)) throw new ArgumentException("Weights path cannot be empty", nameof(path));
        NcMi355x.Check(NcMi355x.nc_codec_load_weights(_h, path));                   // NC_ENOTFOUND -> FileNotFoundException (DAC.cs:347-350)
    }

    // ---- host-array cores (what every overload below marshals into) ---------------------------------------------------------------
    /// <summary>audio [B,1,T] -> (zQ [B,latent,T'], codes [B,nQ,T'], latents [B,nQ*codebookDim,T']); Models/DAC.cs:163-181.</summary>
    public (float[] z, long[] codes, float[] latents, long frames, int nQ) EncodeHost(float[] audio, int B, long T, int? nQuantizers = null,
                                                                                         int? sampleRate = null)
    {
        ArgumentNullException.ThrowIfNull(audio);
        long padded, frames;
        NcMi355x.Check(NcMi355x.nc_dac_query(_h, T, &padded, &frames));
        int nq = (nQuantizers is int n && n > 0 && n <= _config.NumCodebooks) ? n : _config.NumCodebooks;
        var z = new float[(long)B * _latentDim * frames];
        var codes = new long[(long)B * nq * frames];
        var lat = new float[(long)B * nq * _config.CodebookDim * frames];
        fixed (float* p = audio, pz = z, pl = lat) fixed (long* pc = codes)         // sample-rate mismatch -> NC_EINVAL -> ArgumentException (DAC.cs:144-149)
            NcMi355x.Check(NcMi355x.nc_dac_encode(_h, p, B, T, sampleRate ?? 0, nQuantizers ?? 0, pc, pz, pl));
        return (z, codes, lat, frames, nq);
    }

    public float[] DecodeHost(float[] qAudio, int B, long frames)                   // Models/DAC.cs:231-234 on host arrays
    {
        ArgumentNullException.ThrowIfNull(qAudio);
        var pcm = new float[(long)B * frames * _hopLength];
        fixed (float* pz = qAudio, pp = pcm)
            NcMi355x.Check(NcMi355x.nc_dac_decode(_h, pz, B, frames, pp));
        return pcm;
    }

    public float[] FromCodesHost(long[] codes, int B, int nQ, long frames)          // Models/DAC.cs:101-106 on host arrays
    {
        ArgumentNullException.ThrowIfNull(codes);
        var z = new float[(long)B * _latentDim * frames];
        fixed (long* pc = codes) fixed (float* pz = z)
            NcMi355x.Check(NcMi355x.nc_dac_from_codes(_h, pc, B, nQ, frames, pz));
        return z;
    }

    /// <summary>latents [B,cLat,T'] -> (zQ [B,latent,T'], projected [B,nQ*codebookDim,T'], codes [B,nQ,T']) with
    /// nQ = min(NumCodebooks, cLat / CodebookDim); Modules/DAC/ResidualVectorQuantizer.cs:243-300 on host arrays.</summary>
    public (float[] z, float[] projected, long[] codes, int nQ) FromLatentsHost(float[] latents, int B, int cLat, long frames)
    {
        ArgumentNullException.ThrowIfNull(latents);
        int nq = Math.Max(1, Math.Min(_config.NumCodebooks, cLat / _config.CodebookDim));   // (cLat < CodebookDim: NC_EINVAL -> ArgumentException)
        var z = new float[(long)B * _latentDim * frames];
        var proj = new float[(long)B * nq * _config.CodebookDim * frames];
        var codes = new long[(long)B * nq * frames];
        fixed (float* pl = latents, pz = z, pp = proj) fixed (long* pc = codes)
            NcMi355x.Check(NcMi355x.nc_dac_from_latents(_h, pl, B, cLat, frames, pz, pp, pc));
        return (z, proj, codes, nq);
    }

    // ---- the reference's members, signature for signature ---------------------------------------------------------------------------
    public Tensor FromCodes(Tensor codes)                                           // Models/DAC.cs:101-106: codes [B,nQ,T'] int64
    {
        int B = (int)codes.shape[0], nQ = (int)codes.shape[1];
        long frames = codes.shape[2];
        return NcTensor.From(FromCodesHost(NcTensor.Longs(codes), B, nQ, frames), B, _latentDim, frames);
    }

    /// <summary>The quantizer's FromLatents (the reference reaches it as Quantizer.FromLatents): latents [B,C,T'] float32.</summary>
    public (Tensor zQ, Tensor projected, Tensor codes) FromLatents(Tensor latents)  // Modules/DAC/ResidualVectorQuantizer.cs:243-300
    {
        int B = (int)latents.shape[0], cLat = (int)latents.shape[1];
        long frames = latents.shape[2];
        var (z, proj, codes, nq) = FromLatentsHost(NcTensor.Floats(latents), B, cLat, frames);
        return (NcTensor.From(z, B, _latentDim, frames), NcTensor.From(proj, B, (long)nq * _config.CodebookDim, frames),
                NcTensor.From(codes, B, nq, frames));
    }

    public (Tensor z, Tensor codes, Tensor latents, Tensor commitmentLoss, Tensor codebookLoss)
        Encode(Tensor audioData, int? nQuantizers = null, int? sampleRate = null)  // Models/DAC.cs:163-181
    {
        int B = (int)audioData.shape[0];
        long T = audioData.shape[^1];
        var (z, codes, lat, frames, nq) = EncodeHost(NcTensor.Floats(audioData), B, T, nQuantizers, sampleRate);
        return (NcTensor.From(z, B, _latentDim, frames), NcTensor.From(codes, B, nq, frames),
                NcTensor.From(lat, B, (long)nq * _config.CodebookDim, frames),
                torch.zeros(1), torch.zeros(1));                                    // eval mode: both losses are 0 (ResidualVectorQuantizer.cs:143-156)
    }

    public Tensor EncodeAudio(Tensor audioData) => Encode(audioData).z;             // Models/DAC.cs:188-198

    public float[] Encode(float[] audioData)                                        // Models/DAC.cs:205-224: returns the zQ latents (D12)
    {
        ArgumentNullException.ThrowIfNull(audioData);
        return EncodeHost(audioData, 1, audioData.Length).z;
    }

    public Tensor Decode(Tensor qAudio)                                             // Models/DAC.cs:231-234: z [B,latent,T'] -> [B,1,T'*hop]
    {
        int B = (int)qAudio.shape[0];
        long frames = qAudio.shape[2];
        return NcTensor.From(DecodeHost(NcTensor.Floats(qAudio), B, frames), B, 1, frames * _hopLength);
    }

    public float[] Decode(float[] qAudio)                                           // Models/DAC.cs:241-253: reshape(1, latent, -1)
    {
        ArgumentNullException.ThrowIfNull(qAudio);
        return DecodeHost(qAudio, 1, qAudio.Length / _latentDim);
    }

    public Dictionary<string, Tensor> forward(Tensor audioData, int? sampleRate, int? nQuantizers)   // Models/DAC.cs:262-281
    {
        var (z, codes, latents, commitmentLoss, codebookLoss) = Encode(audioData, nQuantizers, sampleRate);
        var audio = Decode(z);
        return new Dictionary<string, Tensor>
        {
            ["audio"] = audio, ["z"] = z, ["codes"] = codes, ["latents"] = latents,
            ["vq/commitment_loss"] = commitmentLoss, ["vq/codebook_loss"] = codebookLoss,
        };
    }

    public Dictionary<string, Tensor> forward(Tensor audioData) => forward(audioData, null, null);   // Models/DAC.cs:288-303

    public float[] forward(float[] audioData)                                       // Models/DAC.cs:310-322
    {
        ArgumentNullException.ThrowIfNull(audioData);
        return Decode(Encode(audioData));
    }

    /// <summary>Dia glue (Models/Dia.cs:973-981, Modules/Dia/AudioUtils.cs:189-199): codes [B,T',n_q] -> PCM [B,1,T'*hop].</summary>
    public float[] DecodeCodeMatrix(long[] codesTq, int B, long frames, int nQ)   // Models/Dia.cs:973-981
    {
        ArgumentNullException.ThrowIfNull(codesTq);
        var pcm = new float[(long)B * frames * _hopLength];
        fixed (long* pc = codesTq) fixed (float* pp = pcm)
            NcMi355x.Check(NcMi355x.nc_dac_decode_code_matrix(_h, pc, B, frames, nQ, pp));
        return pcm;
    }

    /// <summary>Dia glue (Models/Dia.cs:989-1002): audio [B,1,T] -> codes [B,T',n_q].</summary>
    public long[] EncodeCodeMatrix(float[] audio, int B, long T)                   // Models/Dia.cs:989-1002
    {
        ArgumentNullException.ThrowIfNull(audio);
        long padded, frames;
        NcMi355x.Check(NcMi355x.nc_dac_query(_h, T, &padded, &frames));
        var codes = new long[(long)B * frames * _config.NumCodebooks];
        fixed (float* p = audio) fixed (long* pc = codes)
            NcMi355x.Check(NcMi355x.nc_dac_encode_code_matrix(_h, p, B, T, 0, pc));
        return codes;
    }

    /// <summary>Clips of unequal lengths in one call: pcmPacked holds clip b behind clip b-1 (lengths[b] samples each); returns the packed
    /// codes, clip b as [nQ, frames[b]] row-major.  Clip b's codes are those of Encode on that clip alone, bit for bit.</summary>
    public long[] EncodeRagged(float[] pcmPacked, long[] lengths, int nQ, out long[] frames)
    {
        ArgumentNullException.ThrowIfNull(pcmPacked);
        ArgumentNullException.ThrowIfNull(lengths);
        frames = new long[lengths.Length];
        int rows = nQ <= 0 || nQ > _config.NumCodebooks ? _config.NumCodebooks : nQ;
        fixed (long* pl = lengths) fixed (long* pf = frames)
            NcMi355x.Check(NcMi355x.nc_dac_ragged_query(_h, lengths.Length, pl, pf, null));
        long total = 0;
        foreach (long f in frames) total += rows * f;
        var codes = new long[total];
        fixed (float* p = pcmPacked) fixed (long* pl = lengths) fixed (long* pc = codes)
            NcMi355x.Check(NcMi355x.nc_dac_encode_ragged(_h, p, lengths.Length, pl, 0, nQ, pc));
        return codes;
    }

    /// <summary>FromCodes then Decode of clips of unequal lengths in one call: codesPacked as EncodeRagged returns it; the packed PCM holds
    /// decodedLens[b] samples per clip.</summary>
    public float[] DecodeRagged(long[] codesPacked, long[] frames, int nQ, out long[] decodedLens)
    {
        ArgumentNullException.ThrowIfNull(codesPacked);
        ArgumentNullException.ThrowIfNull(frames);
        var lens = new long[frames.Length];
        decodedLens = new long[frames.Length];
        for (int b = 0; b < frames.Length; ++b) lens[b] = (frames[b] - 1) * _hopLength + 1;   // any length with frames[b] frames
        fixed (long* pl = lens) fixed (long* pd = decodedLens)
            NcMi355x.Check(NcMi355x.nc_dac_ragged_query(_h, frames.Length, pl, null, pd));
        long total = 0;
        foreach (long n in decodedLens) total += n;
        var pcm = new float[total];
        fixed (long* pc = codesPacked) fixed (long* pf = frames) fixed (float* pp = pcm)
            NcMi355x.Check(NcMi355x.nc_dac_decode_codes_ragged(_h, pc, frames.Length, pf, nQ, pp));
        return pcm;
    }

    /// <summary>Dia.GenerateOutput on host arrays: delayed codes [B, tGen, C] and the valid length of every item -> the packed waveforms,
    /// outLens[b] samples per item.  The delay pattern is undone, the last max(delay) steps cut, codes outside [minValid, maxValid] set
    /// to 0, all items decoded as one ragged batch and, with speed (one factor per item, null: none), stretched as Dia.AdjustSpeed does.</summary>
    public float[] DecodeDiaOutput(long[] codesDelayed, int B, long tGen, int[] delayPattern, long[] lengths, float[]? speed, out long[] outLens,
                                   long minValid = 0, long maxValid = 1023)   // Models/Dia.cs:1010-1093
    {
        ArgumentNullException.ThrowIfNull(codesDelayed);
        ArgumentNullException.ThrowIfNull(delayPattern);
        ArgumentNullException.ThrowIfNull(lengths);
        outLens = new long[lengths.Length];
        int C = delayPattern.Length;
        fixed (int* pd = delayPattern) fixed (long* pl = lengths, po = outLens) fixed (float* ps = speed)
            NcMi355x.Check(NcMi355x.nc_dia_output_query(_h, B, tGen, C, pd, pl, ps, null, null, po));
        long total = 0;
        foreach (long n in outLens) total += n;
        var pcm = new float[total];
        fixed (long* pc = codesDelayed, pl = lengths) fixed (int* pd = delayPattern) fixed (float* ps = speed, pp = pcm)
            NcMi355x.Check(NcMi355x.nc_dia_decode_output(_h, pc, B, tGen, C, pd, pl, minValid, maxValid, ps, pp));
        return pcm;
    }

    /// <summary>AudioUtils.ApplyAudioDelay on DEVICE arrays (int64 [B, T, C], asynchronous on hipStream): the voice prompt delayed with BOS fill.</summary>
    public void ApplyAudioDelay(IntPtr codesDev, int B, long T, int[] delayPattern, long padValue, long bosValue, IntPtr outDev, IntPtr hipStream)
    {
        ArgumentNullException.ThrowIfNull(delayPattern);
        fixed (int* pd = delayPattern)
            NcMi355x.Check(NcMi355x.nc_dia_apply_delay_dev(NcMi355x.DeviceIndex(_config.Device), (long*)codesDev, B, T, delayPattern.Length, pd, padValue,
                                                           bosValue, (long*)outDev, (void*)hipStream));
    }

    /// <summary>Dia.PrepareAudioPrompt on DEVICE arrays (asynchronous on hipStream): the packed codes of EncodeRagged (item b as
    /// [C, frames[b]] int64, 0 frames: no prompt) -> the delayed prefill int32 [B, tMax, C] with its BOS rows and -1 fill, in one launch per
    /// 32 items.  tMax >= max(frames) + max(delay); padValue is taken as ApplyAudioDelay takes it and never written.</summary>
    public void PrefillPack(IntPtr codesPackedDev, long[] frames, int[] delayPattern, long bosValue, long padValue, long tMax, IntPtr outDev, IntPtr hipStream)   // Models/Dia.cs:329-400
    {
        ArgumentNullException.ThrowIfNull(frames);
        ArgumentNullException.ThrowIfNull(delayPattern);
        fixed (long* pf = frames) fixed (int* pd = delayPattern)
            NcMi355x.Check(NcMi355x.nc_dia_prefill_pack_dev(NcMi355x.DeviceIndex(_config.Device), (long*)codesPackedDev, frames.Length, pf, delayPattern.Length,
                                                            pd, bosValue, padValue, tMax, (int*)outDev, (void*)hipStream));
    }

    /// <summary>Dia.LoadAudio's mono mix, Dia.Encode of every prompt and Dia.PrepareAudioPrompt on host arrays: pcmPacked holds prompt b behind
    /// prompt b-1, lengths[b] frames of channels[b] interleaved samples (0: no prompt; channels null: all mono); lengths.Length is
    /// PrepareAudioPrompt's batch.  Returns the delayed prefill int32 [B, tMax, C] and the prefill steps.  The prompts are not resampled:
    /// the reference discards its resampled copy (Models/Dia.cs:870-874).</summary>
    public int[] EncodeDiaPrompts(float[] pcmPacked, long[] lengths, int[]? channels, int[] delayPattern, int bosValue, out int[] prefillSteps,
                                  out long tMax, int padValue = -1)   // Models/Dia.cs:329-400
    {
        ArgumentNullException.ThrowIfNull(pcmPacked);
        ArgumentNullException.ThrowIfNull(lengths);
        ArgumentNullException.ThrowIfNull(delayPattern);
        int B = lengths.Length, C = delayPattern.Length;
        prefillSteps = new int[B];
        long t;
        fixed (int* pd = delayPattern) fixed (long* pl = lengths)
            NcMi355x.Check(NcMi355x.nc_dia_prompt_query(_h, B, C, pd, pl, null, null, &t));
        tMax = t;
        var prefill = new int[(long)B * t * C];
        fixed (float* pp = pcmPacked) fixed (long* pl = lengths) fixed (int* pc = channels, pd = delayPattern, po = prefill, ps = prefillSteps)
            NcMi355x.Check(NcMi355x.nc_dia_encode_prompts(_h, pp, B, pl, pc, C, pd, bosValue, padValue, po, ps));
        return prefill;
    }

    /// <summary>AudioUtils.RevertAudioDelay with the cut and the mask of Dia.GenerateOutput on DEVICE arrays: [B, T, C] -> [B, T - max(delay), C].</summary>
    public void RevertAudioDelay(IntPtr codesDev, int B, long T, int[] delayPattern, IntPtr outDev, IntPtr hipStream, long minValid = 0, long maxValid = 1023)
    {
        ArgumentNullException.ThrowIfNull(delayPattern);
        fixed (int* pd = delayPattern)
            NcMi355x.Check(NcMi355x.nc_dia_revert_delay_dev(NcMi355x.DeviceIndex(_config.Device), (long*)codesDev, B, T, delayPattern.Length, pd, minValid,
                                                            maxValid, (long*)outDev, (void*)hipStream));
    }

    /// <summary>Dia.AdjustSpeed on rows of packed PCM on the DEVICE: row b of lens[b] samples -> AdjustSpeedLen(lens[b], speed[b]) samples.</summary>
    public void AdjustSpeed(IntPtr pcmPackedDev, long[] lens, float[] speed, IntPtr outPackedDev, IntPtr hipStream)   // Models/Dia.cs:947-966
    {
        ArgumentNullException.ThrowIfNull(lens);
        ArgumentNullException.ThrowIfNull(speed);
        fixed (long* pl = lens) fixed (float* ps = speed)
            NcMi355x.Check(NcMi355x.nc_dia_adjust_speed_dev(NcMi355x.DeviceIndex(_config.Device), (float*)pcmPackedDev, lens.Length, pl, ps,
                                                            (float*)outPackedDev, (void*)hipStream));
    }

    /// <summary>`(int)(L / speed)` with AdjustSpeed's early returns: the samples AdjustSpeed yields for a row of L.</summary>
    public static long AdjustSpeedLen(long L, float speed) => NcMi355x.nc_dia_adjust_speed_len(L, speed);

    private static NcDiaSampleParams SampleParams(float cfgScale, float temperature, float topP, int topK, int eosValue, int padValue) =>
        new NcDiaSampleParams { cfg_scale = cfgScale, temperature = temperature, top_p = topP, top_k = topK, eos = eosValue, pad = padValue };

    /// <summary>Dia.DecoderStep from the logits on (guidance, masks, SampleNextToken) on HOST arrays, no device: logits float32 [2B, C, V]
    /// (row 2b unconditional, 2b + 1 conditional), uniform [B, C] in [0, 1) the draw of every row -> tokens [B, C]; bad[b] != 0: a row of
    /// item b has no token (-1).  The same bits as SampleNextTokenDevice.</summary>
    public static long[] SampleNextTokenHost(float[] logits, int B, int C, int V, float[] uniform, float cfgScale, float temperature, float topP,
                                             int topK, int eosValue, out int[] bad)   // Models/Dia.cs:424-501
    {
        ArgumentNullException.ThrowIfNull(logits);
        ArgumentNullException.ThrowIfNull(uniform);
        if (B <= 0 || C <= 0 || V <= 0 || logits.LongLength != 2L * B * C * V || uniform.LongLength != (long)B * C)
            throw new ArgumentException("logits must be [2B, C, V] and uniform [B, C]");
        var tokens = new long[(long)B * C];
        bad = new int[B];
        var p = SampleParams(cfgScale, temperature, topP, topK, eosValue, eosValue + 1);
        fixed (float* pl = logits, pu = uniform) fixed (long* pt = tokens) fixed (int* pb = bad)
            NcMi355x.Check(NcMi355x.nc_dia_sample_host(pl, B, C, V, p, pu, pt, pb));
        return tokens;
    }

    /// <summary>The same on DEVICE arrays in one launch (asynchronous on hipStream): tokensDev int64 [B, C], badDev int32 [B].</summary>
    public void SampleNextTokenDevice(IntPtr logitsDev, int B, int C, int V, IntPtr uniformDev, float cfgScale, float temperature, float topP, int topK,
                                      int eosValue, IntPtr tokensDev, IntPtr badDev, IntPtr hipStream)   // Models/Dia.cs:530-560
    {
        var p = SampleParams(cfgScale, temperature, topP, topK, eosValue, eosValue + 1);
        NcMi355x.Check(NcMi355x.nc_dia_sample_dev(NcMi355x.DeviceIndex(_config.Device), (float*)logitsDev, B, C, V, p, (float*)uniformDev,
                                                  (long*)tokensDev, (int*)badDev, (void*)hipStream));
    }

    /// <summary>The per-item EOS state of a generation, DEVICE int64 [3, B]: detected 0, countdown -1, finished -1 (Dia.cs:667-669).</summary>
    public void GenerateStateInit(int B, IntPtr stateDev, IntPtr hipStream)   // Models/Dia.cs:667-669
    {
        NcMi355x.Check(NcMi355x.nc_dia_generate_state_init_dev(NcMi355x.DeviceIndex(_config.Device), B, (long*)stateDev, (void*)hipStream));
    }

    /// <summary>One generation step behind the language model in ONE launch: sampling, the EOS countdown of Dia.Generate and
    /// DecoderOutput.UpdateOne into generatedDev int32 [B, L, C] at `step` (the reference's currentStepIdx); applyMask = !bosOver.
    /// activeDev int32 [B] receives countdown != 0; badDev int32 [B] is ORed into (zero it first).  No synchronisation.</summary>
    public void GenerateStep(IntPtr logitsDev, int B, int V, IntPtr uniformDev, int[] delayPattern, float cfgScale, float temperature, float topP, int topK,
                             int eosValue, int padValue, long step, long maxTokens, bool applyMask, IntPtr stateDev, IntPtr generatedDev, long L,
                             IntPtr activeDev, IntPtr badDev, IntPtr hipStream)   // Models/Dia.cs:688-756
    {
        ArgumentNullException.ThrowIfNull(delayPattern);
        var p = SampleParams(cfgScale, temperature, topP, topK, eosValue, padValue);
        fixed (int* pd = delayPattern)
            NcMi355x.Check(NcMi355x.nc_dia_generate_step_dev(NcMi355x.DeviceIndex(_config.Device), (float*)logitsDev, B, delayPattern.Length, V, p,
                                                             (float*)uniformDev, pd, step, maxTokens, applyMask ? 1 : 0, (long*)stateDev,
                                                             (int*)generatedDev, L, (int*)activeDev, (int*)badDev, (void*)hipStream));
    }

    /// <summary>The lengths of Dia.Generate from a host copy of the finished steps (the third row of the state): host arithmetic.</summary>
    public static long[] GenerateLengths(long[] finished, int[] prefillSteps, long finalStep, long maxDelay, out long tGen)   // Models/Dia.cs:775-782
    {
        ArgumentNullException.ThrowIfNull(finished);
        ArgumentNullException.ThrowIfNull(prefillSteps);
        if (finished.Length != prefillSteps.Length) throw new ArgumentException("one finished step and one prefill step per item");
        var lengths = new long[finished.Length];
        long t = 0;
        fixed (long* pf = finished, pl = lengths) fixed (int* pp = prefillSteps)
            NcMi355x.Check(NcMi355x.nc_dia_generate_lengths(finished.Length, pf, pp, finalStep, maxDelay, pl, &t));
        tGen = t;
        return lengths;
    }

    /// <summary>The copy into generatedCodes on DEVICE arrays: generatedDev int32 [B, L, C] -> outDev int64 [B, max(lengths) + maxDelay, C],
    /// the codesDelayed of DecodeDiaOutput with these lengths.</summary>
    public void GenerateCollect(IntPtr generatedDev, long L, int C, int[] prefillSteps, long[] lengths, long maxDelay, long padValue, IntPtr outDev,
                                IntPtr hipStream)   // Models/Dia.cs:786-801
    {
        ArgumentNullException.ThrowIfNull(prefillSteps);
        ArgumentNullException.ThrowIfNull(lengths);
        if (lengths.Length != prefillSteps.Length) throw new ArgumentException("one length and one prefill step per item");
        fixed (int* pp = prefillSteps) fixed (long* pl = lengths)
            NcMi355x.Check(NcMi355x.nc_dia_generate_collect_dev(NcMi355x.DeviceIndex(_config.Device), (int*)generatedDev, lengths.Length, L, C, pp, pl,
                                                                maxDelay, padValue, (long*)outDev, (void*)hipStream));
    }

    /// <summary>Codes pushed as a model emits them (Dia): every push returns the PCM that became final; concatenated, the pieces are
    /// Decode(FromCodes(all codes)), bit for bit.  Dispose the session before the model.</summary>
    public NcSession DecodeSession(int batch, int? nQuantizers = null)
    {
        NcMi355x.Check(NcMi355x.nc_session_create(_h, 1, batch, nQuantizers ?? 0, out IntPtr s));
        return new NcSession(s, batch);
    }

    /// <summary>PCM pushed as it is recorded: every push returns the codes [batch, NumCodebooks, n] that became final.</summary>
    public NcSession EncodeSession(int batch)
    {
        NcMi355x.Check(NcMi355x.nc_session_create(_h, 0, batch, 0, out IntPtr s));
        return new NcSession(s, batch * _config.NumCodebooks);
    }

    /// <summary>slots independent decode streams stepped together (NcSessionPool.StepCodes): every slot as a DecodeSession(1, nQuantizers).</summary>
    public NcSessionPool DecodePool(int slots, int? nQuantizers = null)
    {
        NcMi355x.Check(NcMi355x.nc_session_pool_create(_h, 1, slots, nQuantizers ?? 0, out IntPtr p));
        return new NcSessionPool(p, 1);
    }

    /// <summary>slots independent encode streams stepped together (NcSessionPool.StepAudio): every slot as an EncodeSession(1).</summary>
    public NcSessionPool EncodePool(int slots)
    {
        NcMi355x.Check(NcMi355x.nc_session_pool_create(_h, 0, slots, 0, out IntPtr p));
        return new NcSessionPool(p, _config.NumCodebooks);
    }

    public void Dispose()                                                           // Models/DAC.cs:329-338
    {
        if (_h != IntPtr.Zero) { NcMi355x.nc_codec_destroy(_h); _h = IntPtr.Zero; }
        GC.SuppressFinalize(this);
    }

    ~DACNative() { if (_h != IntPtr.Zero) NcMi355x.nc_codec_destroy(_h); }
}
